// cusz_amd/csrc/quality.hip -- quality assessment of a reconstruction against its original in one
// pass (include/cusz_amd.h psz_amd_assess_quality_*): each array is read once.  The record, what a
// lane does per pair and the combine are quality_reduce.hh's; here are the loads, the partition
// and the reduction across lanes (shuffles), waves (LDS) and workgroups (a partials buffer and one
// small combine launch, as launch_extrema).  No atomics: the combine order is a function of the
// length alone (of the box, for a region), so a result is reproducible bit for bit.
#include <hip/hip_runtime.h>

#include "kernels.hh"
#include "quality_reduce.hh"

namespace cusz_amd {

namespace {

__device__ __forceinline__ double shd(double v, int d) { return __shfl_down(v, d); }
__device__ __forceinline__ uint64_t shd(uint64_t v, int d) { return (uint64_t)__shfl_down((unsigned long long)v, d); }
__device__ __forceinline__ QrMoments shd(const QrMoments& m, int d)
{
  return QrMoments{shd(m.n, d), shd(m.ma, d), shd(m.mb, d), shd(m.M2a, d), shd(m.M2b, d), shd(m.C, d)};
}

// the record a reduction carries: with the autocorrelation pairs only where they are asked for
template <bool AC>
struct Rec;
template <>
struct Rec<false> { using type = QrCore; };
template <>
struct Rec<true> { using type = QrPart; };

// the record of lane + d (lanes past the wave's end read their own: lane 0's tree never uses them)
__device__ __forceinline__ void shd_rec(const QrCore& p, int d, QrCore& q)
{
  q.m = shd(p.m, d);
  q.omin = shd(p.omin, d), q.omax = shd(p.omax, d), q.xmin = shd(p.xmin, d), q.xmax = shd(p.xmax, d);
  q.max_e = shd(p.max_e, d), q.max_pw = shd(p.max_pw, d), q.sum_e2 = shd(p.sum_e2, d);
  q.max_e_idx = shd(p.max_e_idx, d), q.n_unb = shd(p.n_unb, d);
  q.first_unb = shd(p.first_unb, d), q.first_diff = shd(p.first_diff, d);
}
__device__ __forceinline__ void shd_rec(const QrPart& p, int d, QrPart& q)
{
  shd_rec(static_cast<const QrCore&>(p), d, static_cast<QrCore&>(q));
  q.a1 = shd(p.a1, d), q.a2 = shd(p.a2, d);
}

// lanes -> wave (lane 0 takes lane d's record for d = 32, 16, ... 1, each the sum of its own
// subtree) -> workgroup (waves 0 .. NW - 1 in order); thread 0 stores the workgroup's record
template <int NW, typename R>
__device__ __forceinline__ void block_reduce_store(R& p, QrPart* dst)
{
  __shared__ R s_wave[NW];
#pragma unroll
  for (int d = kQrWave / 2; d > 0; d >>= 1) {
    R q;
    shd_rec(p, d, q);
    qr_combine(p, q);
  }
  const int lane = threadIdx.x & (kQrWave - 1), wid = threadIdx.x / kQrWave;
  if (lane == 0) s_wave[wid] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) qr_combine(p, s_wave[w]);
    *static_cast<R*>(dst) = p;
  }
}

__device__ __forceinline__ void lane_record(const QrLane& L, const QrShift&, const QrShift&, QrCore& p) { qr_lane_core(L, p); }
__device__ __forceinline__ void lane_record(const QrLane& L, const QrShift& a1, const QrShift& a2, QrPart& p)
{
  qr_lane_part(L, a1, a2, p);
}
__device__ __forceinline__ void record_init(QrCore& p) { qr_core_init(p); }
__device__ __forceinline__ void record_init(QrPart& p) { qr_part_init(p); }

// an item: kQrVecs 16-byte loads in flight per array where the array is 16-byte aligned (a
// kernel-uniform test, each array for itself), else element by element
template <typename T, int I>
__device__ __forceinline__ void load_item(const T* p, bool aligned, T* v)
{
  if (aligned) {
    const uint4* p4 = reinterpret_cast<const uint4*>(p);
    uint4 a[kQrVecs];
#pragma unroll
    for (int k = 0; k < kQrVecs; k++) a[k] = p4[k];
#pragma unroll
    for (int k = 0; k < kQrVecs; k++) __builtin_memcpy(&v[k * (I / kQrVecs)], &a[k], kQrVecBytes);
  }
  else {
#pragma unroll
    for (int k = 0; k < I; k++) v[k] = p[k];
  }
}

template <typename T, bool AC>
__global__ void __launch_bounds__(kQrBlock) k_quality(const T* __restrict__ x, const T* __restrict__ o, uint64_t len,
                                                      double thr, QrPart* __restrict__ parts)
{
  constexpr int I = qr_item_elems(sizeof(T));
  QrLane L;
  QrShift a1, a2;
  qr_lane_init(L);
  qr_shift_init(a1), qr_shift_init(a2);
  const bool o_al = ((uintptr_t)o & (kQrVecBytes - 1)) == 0, x_al = ((uintptr_t)x & (kQrVecBytes - 1)) == 0;
  const uint64_t nitems = len / I, lanes = (uint64_t)gridDim.x * kQrBlock;
  const uint64_t gtid = (uint64_t)blockIdx.x * kQrBlock + threadIdx.x;
  for (uint64_t it = gtid; it < nitems; it += lanes) {
    const uint64_t base = it * I;
    T ov[I + 2], xv[I];
    load_item<T, I>(o + base, o_al, ov);
    load_item<T, I>(x + base, x_al, xv);
    if (AC) {  // the two neighbours past the item: a line the next lane loads anyway
#pragma unroll
      for (int k = 0; k < 2; k++) ov[I + k] = base + I + k < len ? o[base + I + k] : ov[I - 1];
    }
    qr_lane_add_item<T, I>(L, ov, xv, base, thr);
    if (AC) qr_lag_add_item<T, I>(a1, a2, ov, base, len);
  }
  const uint64_t i = nitems * I + gtid;  // the elements past the last whole item: fewer than I
  if (i < len) {
    qr_lane_add(L, o[i], x[i], i, thr);
    if (AC) {
      if (i + 1 < len) qr_lag_add(a1, (double)o[i], (double)o[i + 1]);
      if (i + 2 < len) qr_lag_add(a2, (double)o[i], (double)o[i + 2]);
    }
  }
  typename Rec<AC>::type p;
  lane_record(L, a1, a2, p);
  block_reduce_store<kQrBlock / kQrWave>(p, parts + blockIdx.x);
}

// The region variant: the reconstruction is a compact box, the original the whole field.  One
// workgroup per run of box rows (as k_crop_box walks them), lanes along x, element by element (a
// box row starts anywhere).  Indices are those of the box.
template <typename T, bool AC>
__global__ void __launch_bounds__(kQrBlock) k_quality_region(const T* __restrict__ xbox, const T* __restrict__ field,
                                                             uint64_t lx, uint64_t ly, uint64_t ox, uint64_t oy,
                                                             uint64_t oz, uint64_t ex, uint64_t ey, uint64_t nrows,
                                                             double thr, QrPart* __restrict__ parts)
{
  QrLane L;
  QrShift a1, a2;
  qr_lane_init(L);
  qr_shift_init(a1), qr_shift_init(a2);
  const uint64_t nbox = nrows * ex;
  auto original = [&](uint64_t j) {  // element j of the box, in the field (the lagged neighbours only)
    const uint64_t row = j / ex, xx = j % ex;
    return field[((oz + row / ey) * ly + oy + row % ey) * lx + ox + xx];
  };
  for (uint64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const T* src = field + ((oz + row / ey) * ly + oy + row % ey) * lx + ox;
    const T* rec = xbox + row * ex;
    for (uint64_t xx = threadIdx.x; xx < ex; xx += kQrBlock) {
      const uint64_t i = row * ex + xx;
      const T ov = src[xx];
      qr_lane_add(L, ov, rec[xx], i, thr);
      if (AC) {
        if (i + 1 < nbox) qr_lag_add(a1, (double)ov, (double)(xx + 1 < ex ? src[xx + 1] : original(i + 1)));
        if (i + 2 < nbox) qr_lag_add(a2, (double)ov, (double)(xx + 2 < ex ? src[xx + 2] : original(i + 2)));
      }
    }
  }
  typename Rec<AC>::type p;
  lane_record(L, a1, a2, p);
  block_reduce_store<kQrBlock / kQrWave>(p, parts + blockIdx.x);
}

// the workgroups' records -> one: thread t of kQrFinalBlock takes records t, t + kQrFinalBlock, ...
// in order, then as above
template <bool AC>
__global__ void __launch_bounds__(kQrFinalBlock) k_quality_final(const QrPart* __restrict__ parts, int nparts,
                                                                 QrPart* __restrict__ out)
{
  using R = typename Rec<AC>::type;
  R p;
  record_init(p);
  for (int i = threadIdx.x; i < nparts; i += kQrFinalBlock) qr_combine(p, static_cast<const R&>(parts[i]));
  block_reduce_store<kQrFinalBlock / kQrWave>(p, out);
}

}  // namespace

template <typename T>
int launch_quality(const T* x, const T* o, size_t len, double thr, bool autocor, QrPart* parts, hipStream_t st)
{
  const uint32_t grid = qr_grid(len, sizeof(T));
  if (autocor) {
    k_quality<T, true><<<grid, kQrBlock, 0, st>>>(x, o, len, thr, parts);
    k_quality_final<true><<<1, kQrFinalBlock, 0, st>>>(parts, (int)grid, parts + kQrGridCap);
  }
  else {
    k_quality<T, false><<<grid, kQrBlock, 0, st>>>(x, o, len, thr, parts);
    k_quality_final<false><<<1, kQrFinalBlock, 0, st>>>(parts, (int)grid, parts + kQrGridCap);
  }
  return (int)hipGetLastError();
}

template <typename T>
int launch_quality_region(const T* xbox, const T* field, size_t lx, size_t ly, const size_t (&o)[3],
                          const size_t (&e)[3], double thr, bool autocor, QrPart* parts, hipStream_t st)
{
  const size_t nrows = e[1] * e[2];
  if (!nrows || !e[0]) return (int)hipErrorInvalidValue;
  const uint32_t grid = qr_region_grid(nrows);
  if (autocor) {
    k_quality_region<T, true><<<grid, kQrBlock, 0, st>>>(xbox, field, lx, ly, o[0], o[1], o[2], e[0], e[1], nrows, thr, parts);
    k_quality_final<true><<<1, kQrFinalBlock, 0, st>>>(parts, (int)grid, parts + kQrGridCap);
  }
  else {
    k_quality_region<T, false><<<grid, kQrBlock, 0, st>>>(xbox, field, lx, ly, o[0], o[1], o[2], e[0], e[1], nrows, thr, parts);
    k_quality_final<false><<<1, kQrFinalBlock, 0, st>>>(parts, (int)grid, parts + kQrGridCap);
  }
  return (int)hipGetLastError();
}

template int launch_quality<float>(const float*, const float*, size_t, double, bool, QrPart*, hipStream_t);
template int launch_quality<double>(const double*, const double*, size_t, double, bool, QrPart*, hipStream_t);
template int launch_quality_region<float>(const float*, const float*, size_t, size_t, const size_t (&)[3],
                                          const size_t (&)[3], double, bool, QrPart*, hipStream_t);
template int launch_quality_region<double>(const double*, const double*, size_t, size_t, const size_t (&)[3],
                                           const size_t (&)[3], double, bool, QrPart*, hipStream_t);

}  // namespace cusz_amd
