// tests/host/quality_reduce_shim.cc -- quality_reduce.hh on the CPU (g++ alone, no HIP header):
// an array pair walked with the kernel's partition (quality.hip k_quality: items round the grid's
// lanes, the remainder one element each to the first lanes) and reduced in the kernel's order
// (lane d into lane 0 for d = 32 .. 1, waves in order, workgroup records t, t + 256, ... per lane of
// the combine launch, then the same tree).  Every constant comes from the header.
#include <vector>

#include "quality_reduce.hh"

using namespace cusz_amd;

namespace {

// what block_reduce_store leaves in thread 0 of a workgroup of p.size() lanes
QrPart reduce_block(std::vector<QrPart>& p)
{
  const int nw = (int)p.size() / kQrWave;
  for (int w = 0; w < nw; w++)
    for (int d = kQrWave / 2; d > 0; d >>= 1)
      for (int l = 0; l < d; l++) qr_combine(p[w * kQrWave + l], p[w * kQrWave + l + d]);
  QrPart r = p[0];
  for (int w = 1; w < nw; w++) qr_combine(r, p[w * kQrWave]);
  return r;
}

template <typename T>
QrPart assess(const T* x, const T* o, uint64_t len, double thr, bool ac)
{
  constexpr int I = qr_item_elems(sizeof(T));
  const uint32_t grid = qr_grid(len, sizeof(T));
  const uint64_t nitems = len / I, lanes = (uint64_t)grid * kQrBlock;
  std::vector<QrPart> parts(grid), lane(kQrBlock);
  auto lags = [&](QrShift& a1, QrShift& a2, uint64_t i) {
    if (i + 1 < len) qr_lag_add(a1, (double)o[i], (double)o[i + 1]);
    if (i + 2 < len) qr_lag_add(a2, (double)o[i], (double)o[i + 2]);
  };
  for (uint32_t b = 0; b < grid; b++) {
    for (int t = 0; t < kQrBlock; t++) {
      QrLane L;
      QrShift a1, a2;
      qr_lane_init(L);
      qr_shift_init(a1), qr_shift_init(a2);
      const uint64_t gtid = (uint64_t)b * kQrBlock + t;
      for (uint64_t it = gtid; it < nitems; it += lanes) {
        const uint64_t base = it * I;
        T w[I + 2];  // the item's originals and the two after it, as the kernel holds them
        for (int k = 0; k < I + 2; k++) w[k] = o[base + k < len ? base + k : base + I - 1];
        qr_lane_add_item<T, I>(L, o + base, x + base, base, thr);
        if (ac) qr_lag_add_item<T, I>(a1, a2, w, base, len);
      }
      const uint64_t i = nitems * I + gtid;
      if (i < len) {
        qr_lane_add(L, o[i], x[i], i, thr);
        if (ac) lags(a1, a2, i);
      }
      qr_lane_part(L, a1, a2, lane[t]);
    }
    parts[b] = reduce_block(lane);
  }
  std::vector<QrPart> last(kQrFinalBlock);
  for (int t = 0; t < kQrFinalBlock; t++) {
    qr_part_init(last[t]);
    for (uint32_t i = t; i < grid; i += kQrFinalBlock) qr_combine(last[t], parts[i]);
  }
  return reduce_block(last);
}

}  // namespace

extern "C" {

// block, wave, vector bytes, vectors per item, grid cap
void qr_shim_constants(int* out)
{
  out[0] = kQrBlock, out[1] = kQrWave, out[2] = kQrVecBytes, out[3] = kQrVecs, out[4] = kQrGridCap;
}

unsigned qr_shim_grid(size_t len, int elem_bytes) { return qr_grid(len, elem_bytes); }

size_t qr_shim_sizeof(void) { return sizeof(psz_amd_quality); }

int qr_shim_assess(const void* x, const void* o, size_t len, int f64, double eb, int flags, psz_amd_quality* out)
{
  if (!x || !o || !out || !len || !(eb >= 0.0)) return PSZ_AMD_ERR_INVALID_ARG;
  const bool ac = (flags & PSZ_AMD_QUALITY_AUTOCOR) != 0;
  const double thr = eb > 0.0 ? 1.001 * eb : INFINITY;
  const QrPart p = f64 ? assess((const double*)x, (const double*)o, len, thr, ac)
                       : assess((const float*)x, (const float*)o, len, thr, ac);
  qr_to_quality(p, len, eb, ac, out);
  return PSZ_SUCCESS;
}

}  // extern "C"

#ifdef QR_SHIM_MAIN
// stand-alone run (built with -fsanitize=address,undefined on the CPU): odd lengths, both types
#include <cstdio>
int main()
{
  for (size_t n : {1u, 2u, 3u, 7u, 8u, 9u, 1000u, 70001u, (1u << 20) + 37u}) {
    std::vector<float> o(n), x(n);
    std::vector<double> od(n), xd(n);
    uint64_t s = 88172645463325252ull + n;
    for (size_t i = 0; i < n; i++) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      od[i] = 1e4 + 1e-3 * (double)(s % 1000), xd[i] = od[i] + 1e-5 * (double)(s % 7);
      o[i] = (float)od[i], x[i] = (float)xd[i];
    }
    psz_amd_quality q, qd;
    if (qr_shim_assess(x.data(), o.data(), n, 0, 1e-3, PSZ_AMD_QUALITY_AUTOCOR, &q)) return 1;
    if (qr_shim_assess(xd.data(), od.data(), n, 1, 1e-3, 0, &qd)) return 1;
    std::printf("%zu %.17g %.17g %zu %zu\n", n, q.stat.score_MSE, qd.stat.odata.std, q.n_finite, qd.stat.max_err_idx);
  }
  return 0;
}
#endif
