// cusz_amd/csrc/brick_stream.hip -- the single-pass mode of the fused brick compressor (overview:
// brick_device.hh): k_brick3_sample, k_brick3_stream, k_brick3_stream_finish and their launchers.
#include "brick_device.hh"

namespace cusz_amd {

BPROF_UNIT(brick_stream_profile)  // k_brick3_stream's counters (brick_device.hh)

namespace {

// =========================================================================================
// single-pass mode (PSZ_AMD_CODEBOOK_STREAM): sample -> host codebook -> one streaming pass
// =========================================================================================
// North-star pins the quant codes, the outliers and the reconstruction, not the bitstream, so
// the codebook may come from a sample and the field need be read only once:
//  * k_brick3_sample: the exact codes of a systematic 1/16 sample of 32 x 8 x 8 units (four 8^3
//    tiles: the units cycle through every x position and visit every (y, z) tile row), one unit
//    per wave step with all 8 z-rows in flight; its last workgroup hands the histogram to the
//    host (host-mapped), which builds the two-queue book of sample + 1 (every code encodable).
//  * k_brick3_stream: ONE WORKGROUP PER BRICK, wave y owning the brick's y-step y (rows (y, z),
//    z = 0..7): the wave predicts its 8 rows (z-diff and the x-diff inside the 8-wide tiles in
//    registers; the y-diff against wave y - 1's z/x residuals, exchanged through LDS), looks the
//    codewords up and sums each row's bits.  The workgroup's total is the brick's size: wave 0
//    publishes it for the decoupled look-back over the bricks before it while every wave packs
//    its rows into its own LDS area, and once the offset is known each wave writes its rows
//    straight to the archive.  Codes never touch HBM, nothing is staged per brick beyond a
//    y-step's cells, there is no plan pass and no gap between bricks.  Workgroup 0 takes the
//    host's book (a device-polled gate) while every workgroup predicts its first brick.
//  * k_brick3_stream_finish: outlier segment (the per-(brick, y-step) slots in brick order, then
//    the spill list), totals, both headers; the last workgroup publishes the compress summary.
// Deadlock-free: bricks are claimed in ticket order by resident workgroups, a workgroup claims
// its next brick only while working on an earlier one, and a look-back waits only on aggregates
// of smaller tickets -- the smallest unfinished brick always has every predecessor's.
constexpr uint32_t kSampleStride = 16;
constexpr unsigned long long kStAgg = 1ull << 62, kStInc = 2ull << 62;  // look-back status flags

// sample units of 32 x 8 x 8 elements; stride 16 from 4096 units up (>= 256 samples), else all
__host__ __device__ inline uint32_t sample_units(uint32_t lx, uint32_t ly, uint32_t lz)
{
  return (lx / 32u) * ((ly + 7u) / 8u) * ((lz + 7u) / 8u);
}
__host__ __device__ inline uint32_t sample_stride(uint32_t units) { return units >= 256u * kSampleStride ? kSampleStride : 1u; }

template <typename T>
__device__ __forceinline__ T shfl_up8(T v)
{
  if constexpr (sizeof(T) == 4)
    return __builtin_bit_cast(T, __shfl_up(__builtin_bit_cast(int, v), 8));
  else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __shfl_up((int)(uint32_t)u, 8), hi = __shfl_up((int)(uint32_t)(u >> 32), 8);
    return __builtin_bit_cast(T, (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32));
  }
}

constexpr int kSampleThreads = 256;
template <typename T, bool ZZ>
__global__ void __launch_bounds__(kSampleThreads)
k_brick3_sample(const T* __restrict__ in, uint32_t lx, uint32_t ly, uint32_t lz, T ebx2_r, T r,
                uint32_t* __restrict__ g_hist, int bklen, uint32_t* ticket, uint32_t* h_hist, uint32_t* flag,
                uint32_t epoch)
{
  __shared__ uint32_t s_h[kMaxBklen];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < bklen; i += blockDim.x) s_h[i] = 0;
  __syncthreads();
  const uint32_t nux = lx / 32u, nuy = (ly + 7u) / 8u, units = sample_units(lx, ly, lz);
  const uint32_t stride = sample_stride(units), nsamp = (units + stride - 1) / stride;
  const size_t plane = (size_t)lx * ly;
  const uint32_t ly_l = (uint32_t)lane >> 3, xq = (uint32_t)lane & 7u;
  constexpr int kW = kSampleThreads / 64;
  for (uint32_t i = blockIdx.x * kW + wid; i < nsamp; i += gridDim.x * kW) {
    const uint32_t u = i * stride + i % stride;
    if (u >= units) continue;  // (uniform)
    const uint32_t ux = u % nux, t = u / nux, uy = t % nuy, uz = t / nuy;
    const uint32_t y = uy * 8u + ly_l, x0 = ux * 32u + xq * 4u, z0 = uz * 8u;
    T v[8][4];
#pragma unroll
    for (int z = 0; z < 8; z++) {
      const bool ok = y < ly && z0 + (uint32_t)z < lz;
      load_row<T, 4>(in, (size_t)(z0 + z) * plane + (size_t)y * lx, x0, lx, ok, v[z]);
    }
    // prequant, z-diff, x-diff inside the 8-wide tile (two lanes), then the y-diff across lanes
    T a[8][4], pp[4];
#pragma unroll
    for (int z = 0; z < 8; z++) residual_zx(v[z], ebx2_r, z == 0, !(lane & 1), pp, a[z]);
#pragma unroll
    for (int z = 0; z < 8; z++) {
      const bool ok = y < ly && z0 + (uint32_t)z < lz;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const T north = shfl_up8(a[z][k]);
        const T d = lane >= 8 ? a[z][k] - north : a[z][k];
        bool ol;
        float ov;
        const uint16_t c = quantize<T, ZZ>(d, r, ol, ov);
        if (ok) atomicAdd(&s_h[c], 1u);
      }
    }
  }
  // bins one 64-B line apart (kSampleBinStride): the workgroups finish together, and their
  // atomics would queue on the few lines of a dense array
  __syncthreads();
  for (int i = threadIdx.x; i < bklen; i += blockDim.x)
    if (s_h[i]) atomicAdd(&g_hist[i * kSampleBinStride], s_h[i]);
  if (!last_block(ticket)) return;  // the last workgroup: the sample histogram -> the host, flag raised
  for (int i = threadIdx.x; i < bklen; i += blockDim.x)
    h_hist[i] = __hip_atomic_load(g_hist + i * kSampleBinStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ unsigned long long st_word(unsigned long long flag, uint32_t cells, uint32_t oc)
{
  return flag | (unsigned long long)cells | ((unsigned long long)oc << 32);
}

// Exclusive prefix (cells, slot outliers) of `brick` from its predecessors' status words: 256 per
// step (4 per lane, distance 4 lane + q), back to the nearest one holding an inclusive prefix.
// Bounded spins: a word still empty after them counts as 0 and raises *timeout (never expected).
__device__ __forceinline__ void lookback(const unsigned long long* status, uint32_t brick, int lane, uint32_t& xc,
                                         uint32_t& xo, unsigned int* timeout)
{
  uint32_t sc = 0, so = 0;
  for (int64_t j = (int64_t)brick - 1;; j -= 256) {
    unsigned long long v[4];
    uint32_t qinc = 4;  // this lane's nearest inclusive word (4: none)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t me = j - 4 * lane - q;
      v[q] = kStInc;  // before brick 0: an inclusive prefix of 0
      if (me >= 0) {
        uint32_t spins = 0;
        do
          v[q] = __hip_atomic_load(status + me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((v[q] >> 62) == 0 && ++spins < (1u << 22));
        if ((v[q] >> 62) == 0) atomicOr(timeout, 1u);
      }
    }
#pragma unroll
    for (int q = 3; q >= 0; q--)
      if ((v[q] >> 62) == 2) qinc = (uint32_t)q;
    const uint64_t inc = __builtin_amdgcn_ballot_w64(qinc < 4);
    const int k = inc ? __builtin_ctzll(inc) : 64;  // the lane holding the nearest inclusive word
    uint32_t c = 0, o = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const bool take = lane < k || (lane == k && (uint32_t)q <= qinc);
      c += take ? (uint32_t)v[q] : 0u;
      o += take ? (uint32_t)(v[q] >> 32) & 0x3FFFFFFFu : 0u;
    }
    sc += readlane(hfd::wave_incl_scan(c), 63);
    so += readlane(hfd::wave_incl_scan(o), 63);
    if (inc) break;
  }
  xc = sc, xo = so;
}

struct StreamArgs {
  uint32_t lx, ly, lz, nbx, nby, nbricks;
  OutlierSink ol;              // one slot per (brick, y-step): slot 8 brick + y, cap_per_brick = its cap
  uint32_t* book;              // device book: written by workgroup 0 from the host's
  int bklen;
  uint32_t* par_nbit;
  uint32_t* par_entry;
  uint32_t* bitstream;
  uint32_t bs_cap;             // bitstream capacity (cells)
  unsigned long long* status;  // per brick, zeroed per call
  uint32_t* ticket;            // zeroed per call
  uint32_t* ol_dst;            // per slot: its first cell in the archive's outlier segment
  CompressInfo* info;
  unsigned int* timeout;
  // the codebook gate: the host writes the book and reverse book to host-mapped memory and sets
  // *gate = gate_epoch; workgroup 0 copies them to `book` and the archive, then sets *book_flag
  const uint32_t* gate;
  uint32_t gate_epoch;
  const uint32_t* h_book;
  const uint32_t* h_revbook;
  uint32_t* revbook;  // the archive's reverse book
  int rv_words;
  uint32_t* book_flag;  // device word, never reset (epoch-compared)
};

constexpr int kStreamWaves = 8;  // one wave per y-step of the brick
// LDS per workgroup: waves 0..6 hand their y-step's z/x residuals to the next wave (the y-diff)
// through an exchange area; every wave stages its y-step's packed cells in a staging area until
// the brick's offset is known (one brick later: the look-back is deferred)
template <typename T>
constexpr int kStreamXsWords = 8 * kBrickW * (int)sizeof(T) / 4;
constexpr int kStageW = 512;  // staging words per wave
static_assert(kStageW >= 2 * kPackRowMax + 2, "the flush path holds two rows");
template <typename T>
constexpr size_t stream_lds_bytes()
{
  return ((size_t)(kStreamWaves - 1) * kStreamXsWords<T> + (size_t)kStreamWaves * kStageW) * 4;
}
constexpr uint32_t kNoBrick = 0xFFFFFFFFu;

// Single-pass encoder, one workgroup per brick, wave y = the brick's y-step y.  Per brick:
//   phase 1   prequant, z-diff, x-diff of the wave's 8 rows (loaded one brick ahead), residuals
//             -> the exchange area; (A) the next brick's rows are issued, y-diff from the area
//   phase 2   codes, outliers (the y-step's slot), row bits (LDS book), row scans; (B) sizes
//   wave 0    publishes the brick's aggregate, then looks back for the PREVIOUS brick (its
//             predecessors published a brick ago: the walk rarely waits) and publishes its
//             inclusive prefix; (C)
//   all       copy the previous brick's staged cells out, then pack this brick's into staging.
// A brick with a y-step too large for the staging (noisy fields) takes its own offset at once
// and packs through the staging area with flushes.
template <typename T, bool ZZ>
__global__ void __launch_bounds__(64 * kStreamWaves)
__attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 4 : 2)))  // f32: 2 workgroups per CU (LDS, 128 VGPRs)
k_brick3_stream(const T* __restrict__ in, StreamArgs a, T ebx2_r, T r)
{
  constexpr int V = kBrickV, W = kBrickW;
  constexpr int XW = kStreamXsWords<T>;
  extern __shared__ uint32_t smem[];  // exchange areas (waves 0..6), then staging areas
  __shared__ uint32_t s_book[kMaxBklen];
  __shared__ uint32_t s_wc[kStreamWaves], s_wo[kStreamWaves];
  __shared__ uint32_t s_next[2], s_x[4];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* const xsT = reinterpret_cast<T*>(smem + (wid < kStreamWaves - 1 ? wid : 0) * XW);
  const T* const xprev = reinterpret_cast<const T*>(smem + (wid > 0 ? wid - 1 : 0) * XW);
  uint32_t* const stg = smem + (kStreamWaves - 1) * XW + wid * kStageW;
  const StepLoader<T> ld{in, (size_t)a.lx * a.ly, a.lx, a.ly, a.lz, a.nbx, a.nby, a.nbricks, (uint32_t)lane};
  const uint32_t subcap = a.ol.cap_per_brick;

  // workgroup 0, wave 0: the host's codebook -> device memory and the archive, then the flag
  if (blockIdx.x == 0 && wid == 0) {
    uint32_t ok = 1;
    if (lane == 0) {
      for (uint32_t spin = 0;; spin++) {
        const uint32_t v = __hip_atomic_load(a.gate, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((int32_t)(v - a.gate_epoch) >= 0) break;
        if (spin > (1u << 22)) {
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    ok = (uint32_t)__builtin_amdgcn_readfirstlane((int)ok);
    if (!ok && lane == 0) atomicOr(a.timeout, 2u);
    for (int i = lane; i < a.bklen; i += 64) a.book[i] = a.h_book[i];
    for (int i = lane; i < a.rv_words; i += 64) a.revbook[i] = a.h_revbook[i];
    __builtin_amdgcn_s_waitcnt(0);
    hfd::wave_sync();
    if (lane == 0) __hip_atomic_store(a.book_flag, a.gate_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }

  if (threadIdx.x == 0) s_next[0] = atomicAdd(a.ticket, 1u);
  __syncthreads();
  uint32_t brick = s_next[0];
  T q[8][V];  // this wave's rows of the brick (loaded one brick ahead)
  {
    const auto br = ld.rows_of(brick);
#pragma unroll
    for (int z = 0; z < 8; z++) ld.issue_row(br, (uint32_t)wid, (uint32_t)z, q[z]);
  }
  bool have_book = false;
  unsigned long long wbits = 0;  // bits this wave packed (the header's total)
  uint32_t par = 0;
  // the deferred brick (uniform): its index, totals, this wave's cells / slot outliers before it
  // and its own; lane z: its row z's bits and first cell
  uint32_t dbrick = kNoBrick, d_ct = 0, d_ot = 0, d_cb = 0, d_ob = 0, d_cells = 0, d_cnt = 0;
  uint32_t d_nbit = 0, d_loc = 0;
  // diagnostic build: per-phase clocks summed over waves (0 wave-bricks, 1 phase 1 incl. the
  // loads' wait, 2 barrier A + y-diff + book, 3 phase 2, 4 barrier B, 5 look-back (wave 0),
  // 6 barrier C, 7 copy-out of the deferred brick, 8 pack)
  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = 0, tp = __builtin_readcyclecounter();)
#define SPROF(i) BPROF(hfd::wave_sync(); tk = __builtin_readcyclecounter(); pc[i] += tk - tp; tp = tk;)
  for (;;) {
    const bool live = brick < a.nbricks;  // (uniform over the workgroup)
    if (!live && dbrick == kNoBrick) break;
    BPROF(pc[0] += live;)
    const uint32_t bx = brick % a.nbx, t = brick / a.nbx, by = t % a.nby, bz = t / a.nby;
    const uint32_t x0 = bx * W + lane * V, z0 = bz * 8, gy = by * 8 + (uint32_t)wid;
    const bool yok = live && gy < a.ly;  // (uniform per wave)
    const uint32_t nzv = live ? min(8u, a.lz - z0) : 0u;
    const uint32_t slot = brick * kStreamWaves + (uint32_t)wid;
    uint32_t cnt = 0, cells = 0;
    uint32_t cp[8][2], inc[8];  // codes as u16 pairs, row scans of the bits (lane 63: the row's bits)
    bool wide = false;                  // a lane's four codewords of some row exceed 64 bits
    uint32_t bnext = kNoBrick;
    if (live) {
      // phase 1: prequant, z-diff, x-diff inside the 8-wide tile
      T av[8][V], pprev[V];
#pragma unroll
      for (int z = 0; z < 8; z++) residual_zx(q[z], ebx2_r, z == 0, x0 % 8 == 0, pprev, av[z]);
      if (wid < kStreamWaves - 1)
#pragma unroll
        for (int z = 0; z < 8; z++) lds_store4(xsT + ((size_t)z * 64 + lane) * V, av[z]);
      if (threadIdx.x == 0) s_next[par ^ 1] = atomicAdd(a.ticket, 1u);
      SPROF(1)
      __syncthreads();  // (A) residuals exchanged, next brick known
      bnext = s_next[par ^ 1];
      par ^= 1;
      const auto bn = ld.rows_of(bnext);  // (past the last brick: the loads read 0)
#pragma unroll
      for (int z = 0; z < 8; z++) ld.issue_row(bn, (uint32_t)wid, (uint32_t)z, q[z]);
      if (!have_book) {  // first brick: the codebook (workgroup 0 raises the flag)
        if (threadIdx.x == 0) {
          for (uint32_t spin = 0;; spin++) {
            const uint32_t v = __hip_atomic_load(a.book_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (v == a.gate_epoch) break;
            if (spin > (1u << 22)) {
              atomicOr(a.timeout, 2u);
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < a.bklen; i += 64 * kStreamWaves)
          s_book[i] = __hip_atomic_load(a.book + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        have_book = true;
      }
      SPROF(2)
      // phase 2: y-diff against the previous y-step (the brick's first y-step has none), codes
      // (kept as u16 pairs), outliers (into this y-step's slot), row bits
#pragma unroll
      for (int z = 0; z < 8; z++) {
        const bool rok = yok && (uint32_t)z < nzv;
        if (wid > 0) {
          T bp[V];
          lds_load4(xprev + ((size_t)z * 64 + lane) * V, bp);
#pragma unroll
          for (int k = 0; k < V; k++) av[z][k] = av[z][k] - bp[k];
        }
        uint16_t c[V];
        float olv[V];
        uint32_t mask = 0;
#pragma unroll
        for (int k = 0; k < V; k++) {
          bool is_ol;
          c[k] = quantize<T, ZZ>(av[z][k], r, is_ol, olv[k]);
          mask |= (uint32_t)(is_ol && rok) << k;
        }
        if (__builtin_amdgcn_ballot_w64(mask != 0)) {  // (rare; the field has < 2^32 elements)
          const uint32_t base = (uint32_t)((z0 + z) * ld.plane + (size_t)gy * a.lx) + x0;
          emit_outliers32<V>(a.ol, slot, cnt, mask, olv, base);
        }
        uint32_t bits = 0;  // (rows outside the field: no codewords)
#pragma unroll
        for (int k = 0; k < V; k++) bits += rok ? s_book[c[k]] >> 27 : 0u;
        cp[z][0] = (uint32_t)c[0] | (uint32_t)c[1] << 16;
        cp[z][1] = (uint32_t)c[2] | (uint32_t)c[3] << 16;
        wide |= bits > 64u;
        inc[z] = hfd::wave_incl_scan(bits);
        cells += (readlane(inc[z], 63) + 31) >> 5;
      }
      if (lane == 0) s_wc[wid] = cells, s_wo[wid] = min(cnt, subcap);
      SPROF(3)
    }
    __syncthreads();  // (B) every y-step's size; the exchange areas are free
    SPROF(4)
    uint32_t cb = 0, ob = 0, ct = 0, ot = 0, cmax = 0;  // before this wave, brick totals, largest y-step
    if (live) {
#pragma unroll
      for (int v = 0; v < kStreamWaves; v++) {
        const uint32_t c = s_wc[v], o = s_wo[v];
        if (v < wid) cb += c, ob += o;
        ct += c, ot += o;
        cmax = max(cmax, c);
      }
    }
    const bool direct = live && cmax + 2 > (uint32_t)kStageW;  // (uniform) too large to stage: offsets now
    if (wid == 0) {
      if (live && lane == 0)  // the brick's aggregate (brick 0: its inclusive prefix)
        __hip_atomic_store(a.status + brick, st_word(brick == 0 ? kStInc : kStAgg, ct, ot), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      if (dbrick != kNoBrick) {  // the deferred brick's offsets
        uint32_t xc = 0, xo = 0;
        if (dbrick != 0) {
          lookback(a.status, dbrick, lane, xc, xo, a.timeout);
          if (lane == 0)
            __hip_atomic_store(a.status + dbrick, st_word(kStInc, xc + d_ct, xo + d_ot), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_x[0] = xc, s_x[1] = xo;
      }
      if (direct) {  // this brick's offsets at once
        uint32_t xc = 0, xo = 0;
        if (brick != 0) {
          lookback(a.status, brick, lane, xc, xo, a.timeout);
          if (lane == 0)
            __hip_atomic_store(a.status + brick, st_word(kStInc, xc + ct, xo + ot), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_x[2] = xc, s_x[3] = xo;
      }
    }
    SPROF(5)
    __syncthreads();  // (C) the offsets
    SPROF(6)
    // cells -> the archive, with the brick's chunk tables and slot destination
    auto emit = [&](uint32_t b, uint32_t woff, uint32_t oo, uint32_t ncells, uint32_t nbit, uint32_t loc,
                    uint32_t scnt) {
      const uint32_t bxx = b % a.nbx, tt = b / a.nbx, byy = tt % a.nby, bzz = tt / a.nby;
      const uint32_t gyy = byy * 8 + (uint32_t)wid, nz = min(8u, a.lz - bzz * 8);
      if (woff + ncells <= a.bs_cap) {
        for (uint32_t i = (uint32_t)lane; i < ncells; i += 64) a.bitstream[woff + i] = stg[i];
      }
      else if (lane == 0)
        atomicOr(a.timeout, 4u);
      if (lane < 8 && gyy < a.ly && (uint32_t)lane < nz) {
        const size_t c = ((size_t)(bzz * 8 + (uint32_t)lane) * a.ly + gyy) * a.nbx + bxx;
        a.par_nbit[c] = nbit;
        a.par_entry[c] = woff + loc;
      }
      if (lane == 0) {
        const uint32_t s = b * kStreamWaves + (uint32_t)wid;
        a.ol.brick_cnt[s] = scnt;
        a.ol_dst[s] = oo;
        if (scnt > subcap) atomicMax(&a.info->max_brick_cnt, scnt * kStreamWaves);  // slot growth
      }
    };
    if (dbrick != kNoBrick) {
      hfd::wave_sync();
      emit(dbrick, s_x[0] + d_cb, s_x[1] + d_ob, d_cells, d_nbit, d_loc, d_cnt);
      dbrick = kNoBrick;
    }
    SPROF(7)
    if (live) {
      // pack the y-step's rows into the staging area (zeroed first; two words of slack); the
      // codewords are looked up again (fewer registers live across the barriers than holding them)
      const bool any_wide = __builtin_amdgcn_ballot_w64(wide) != 0;
      uint32_t off = 0, fbase = 0, my_nbit = 0, my_loc = 0;  // lane z: row z's bits and first cell
      const uint32_t woff = direct ? s_x[2] + cb : 0u;
      auto flush = [&]() {  // (direct) staged words [fbase, off) -> the archive, staging cleared
        hfd::wave_sync();
        const uint32_t m = off - fbase;
        const bool fits = woff + off <= a.bs_cap;
        if (!fits && lane == 0) atomicOr(a.timeout, 4u);
        for (uint32_t i = (uint32_t)lane; i < m; i += 64) {
          const uint32_t v = stg[i];
          stg[i] = 0u;
          if (fits) a.bitstream[woff + fbase + i] = v;
        }
        fbase = off;
        hfd::wave_sync();
      };
      for (uint32_t i = (uint32_t)lane; i < (direct ? (uint32_t)kStageW : cells + 2); i += 64) stg[i] = 0u;
#pragma unroll
      for (int z = 0; z < 8; z++) {
        if (direct && off - fbase + kPackRowMax > (uint32_t)kStageW) flush();
        uint32_t w[V];
        w[0] = s_book[cp[z][0] & 0xFFFFu], w[1] = s_book[cp[z][0] >> 16];
        w[2] = s_book[cp[z][1] & 0xFFFFu], w[3] = s_book[cp[z][1] >> 16];
        if (!(yok && (uint32_t)z < nzv)) w[0] = w[1] = w[2] = w[3] = 0u;  // a row outside the field (uniform)
        const uint32_t bits = (w[0] >> 27) + (w[1] >> 27) + (w[2] >> 27) + (w[3] >> 27);
        const uint32_t pos = ((off - fbase) << 5) + inc[z] - bits;
        if (!any_wide)
          hfd::pack4_or_lj(stg, pos, w, bits);
        else
          hfd::pack_words<V>(stg, pos, w, V);
        const uint32_t tot = readlane(inc[z], 63);
        if (lane == z) my_nbit = tot, my_loc = off;
        off += (tot + 31) >> 5;
        wbits += tot;
      }
      if (direct) {
        flush();
        emit(brick, woff, s_x[3] + ob, 0u, my_nbit, my_loc, cnt);  // (the cells are out)
      }
      else {
        dbrick = brick, d_ct = ct, d_ot = ot, d_cb = cb, d_ob = ob, d_cells = cells, d_cnt = cnt;
        d_nbit = my_nbit, d_loc = my_loc;
      }
      brick = bnext;
    }
    SPROF(8)
  }
#undef SPROF
  if (lane == 0 && wbits) atomicAdd(&a.info->total_nbit, wbits);
  BPROF(prof_add(pc, lane);)
}

// after the streaming pass: the outlier segment (the slots in (brick, y-step) order -- brick
// order, row order inside a brick -- then the spill list), the totals and both headers; the last
// workgroup publishes the compress summary.  Each wave copies 64 consecutive slots: their
// destinations are one contiguous range, a cell finds its slot by a binary search over the
// slots' prefix counts.
constexpr int kFinishThreads = 256;
__global__ void __launch_bounds__(kFinishThreads) k_brick3_stream_finish(StreamArgs a, HeaderTpl tpl, uint8_t* archive,
                                                                         size_t phf_offset, size_t bits_rel, HostPub pub)
{
  __shared__ uint32_t s_ex[kFinishThreads / 64][65];
  const unsigned long long last =
      __hip_atomic_load(a.status + a.nbricks - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t ncell = (uint32_t)last, slot_total = (uint32_t)(last >> 32) & 0x3FFFFFFFu;
  uint2* ol_dst = reinterpret_cast<uint2*>(a.bitstream + ncell);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t* ex = s_ex[wid];
  const uint32_t nslot = a.nbricks * kStreamWaves, cap = a.ol.cap_per_brick;
  const uint32_t nwv = gridDim.x * (kFinishThreads / 64);
  for (uint32_t g = blockIdx.x * (kFinishThreads / 64) + wid; g * 64 < nslot; g += nwv) {
    const uint32_t s = g * 64 + (uint32_t)lane;
    const uint32_t c = s < nslot ? min(a.ol.brick_cnt[s], cap) : 0u;
    const uint32_t d = s < nslot ? a.ol_dst[s] : 0u;
    const uint32_t incl = hfd::wave_incl_scan(c), total = readlane(incl, 63), d0 = readlane(d, 0);
    ex[lane] = incl - c;
    hfd::wave_sync();
    for (uint32_t j = (uint32_t)lane; j < total; j += 64) {
      uint32_t lo = 0;  // the last slot whose first cell is <= j
#pragma unroll
      for (uint32_t step = 32; step > 0; step >>= 1)
        if (lo + step < 64 && ex[lo + step] <= j) lo += step;
      const uint64_t cell = a.ol.slots[(size_t)(g * 64 + lo) * cap + (j - ex[lo])];
      ol_dst[d0 + j] = make_uint2((uint32_t)cell, (uint32_t)(cell >> 32));
    }
    hfd::wave_sync();
  }
  const uint32_t sp = *a.ol.spill_cnt, sp_kept = min(sp, a.ol.spill_cap);
  for (uint32_t i = blockIdx.x * kFinishThreads + threadIdx.x; i < sp_kept; i += gridDim.x * kFinishThreads) {
    const uint64_t c = a.ol.spill[i];
    ol_dst[slot_total + i] = make_uint2((uint32_t)c, (uint32_t)(c >> 32));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long nbit = __hip_atomic_load(&a.info->total_nbit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.info->total_ncell = ncell;
    a.info->splen = slot_total + sp_kept;
    a.info->outlier_lost = sp > a.ol.spill_cap ? sp - a.ol.spill_cap : 0u;
    a.info->spilled = sp;
    write_headers_dev(archive, tpl, nbit, ncell, slot_total + sp_kept, phf_offset, bits_rel);
    __threadfence();  // the header and totals reach memory before the ticket (the publisher may be another XCD)
  }
  publish_last(pub);
}

}  // namespace

template <typename T>
int launch_brick_sample(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, uint32_t* hist, int bklen,
                        uint32_t* ticket, uint32_t* h_hist, uint32_t* flag, uint32_t epoch, hipStream_t st)
{
  const BrickGeom& g = L.g;
  if (g.ndim != 3 || bklen > kMaxBklen) return (int)hipErrorInvalidValue;
  const T ebx2_r = (T)(1.0 / (eb * 2)), r = (T)radius;
  const uint32_t units = sample_units(L.lx, L.ly, L.lz), stride = sample_stride(units);
  const uint32_t nsamp = (units + stride - 1) / stride;
  constexpr uint32_t kW = kSampleThreads / 64;
  // two sample units per wave on a 512^3 field: half the workgroups' histogram flushes
  const uint32_t grid = std::max(1u, std::min((nsamp + kW - 1) / kW, 2u * (uint32_t)L.ncu));
  if (zz)
    k_brick3_sample<T, true><<<grid, kSampleThreads, 0, st>>>(in, L.lx, L.ly, L.lz, ebx2_r, r, hist, bklen, ticket,
                                                               h_hist, flag, epoch);
  else
    k_brick3_sample<T, false><<<grid, kSampleThreads, 0, st>>>(in, L.lx, L.ly, L.lz, ebx2_r, r, hist, bklen, ticket,
                                                                h_hist, flag, epoch);
  return (int)hipGetLastError();
}

template <typename T>
int launch_brick_stream(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, const BrickSingle& s,
                        const void* psz_tpl, const void* phf_tpl, hipStream_t st, const HostPub& pub)
{
  const BrickGeom& g = L.g;
  if (g.ndim != 3 || s.bklen > kMaxBklen) return (int)hipErrorInvalidValue;
  const T ebx2_r = (T)(1.0 / (eb * 2)), r = (T)radius;
  StreamArgs a{L.lx,        L.ly,   L.lz,         g.nbx,        g.nby,      g.nbricks, s.ol,       s.book,
               s.bklen,     s.par_nbit, s.par_entry, s.bitstream, s.bs_cap, s.status,  s.ticket,   s.ol_dst,
               s.info,      s.timeout, s.gate,     s.gate_epoch, s.h_book,   s.h_revbook, s.revbook, s.rv_words,
               s.book_flag};
  const size_t lds = stream_lds_bytes<T>();  // dynamic: the exchange and staging areas
  static int per_cu[2] = {0, 0};
  int& pc = per_cu[sizeof(T) == 8];
  if (!pc) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, k_brick3_stream<T, false>, 64 * kStreamWaves, lds) !=
            hipSuccess ||
        pc < 1)
      pc = 1;
  }
  // persistent workgroups claim bricks from the ticket; every one must be resident (a look-back
  // waits only on claimed bricks, and workgroup 0 hands every other one the codebook)
  const uint32_t grid = std::max(1u, std::min(g.nbricks, (uint32_t)(pc * L.ncu)));
  if (zz)
    k_brick3_stream<T, true><<<grid, 64 * kStreamWaves, lds, st>>>(in, a, ebx2_r, r);
  else
    k_brick3_stream<T, false><<<grid, 64 * kStreamWaves, lds, st>>>(in, a, ebx2_r, r);
  if (hipError_t e = hipGetLastError()) return (int)e;
  HeaderTpl t;
  __builtin_memcpy(t.psz, psz_tpl, 176);
  __builtin_memcpy(t.phf, phf_tpl, 64);
  const uint32_t nslot_groups = (g.nbricks * kStreamWaves + 63) / 64;
  const uint32_t fgrid = std::max(1u, std::min((nslot_groups + 3) / 4, 1024u));
  k_brick3_stream_finish<<<fgrid, kFinishThreads, 0, st>>>(a, t, s.archive, s.phf_offset, s.bits_rel, pub);
  return (int)hipGetLastError();
}

template int launch_brick_sample<float>(const BrickLaunch&, const float*, double, int, bool, uint32_t*, int,
                                        uint32_t*, uint32_t*, uint32_t*, uint32_t, hipStream_t);
template int launch_brick_sample<double>(const BrickLaunch&, const double*, double, int, bool, uint32_t*, int,
                                         uint32_t*, uint32_t*, uint32_t*, uint32_t, hipStream_t);
template int launch_brick_stream<float>(const BrickLaunch&, const float*, double, int, bool, const BrickSingle&,
                                        const void*, const void*, hipStream_t, const HostPub&);
template int launch_brick_stream<double>(const BrickLaunch&, const double*, double, int, bool, const BrickSingle&,
                                         const void*, const void*, hipStream_t, const HostPub&);

}  // namespace cusz_amd
