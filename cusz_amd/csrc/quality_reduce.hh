// cusz_amd/csrc/quality_reduce.hh -- the record of the quality assessment (include/cusz_amd.h,
// psz_amd_assess_quality_*), what one lane does per element pair, and the combine of two records.
// Host and device, no HIP header: g++ alone compiles it (tests/host/quality_reduce_shim.cc), so
// psz_amd_quality_merge and the CPU tests run the code the kernel (quality.hip) runs.
//
// One pass, no pre-computed mean: a lane keeps SHIFTED sums S(o - K), S(x - K'), S(o - K)^2,
// S(x - K')^2, S(o - K)(x - K') with K, K' the first finite pair it meets (so the squares stay of
// the size of the lane's own spread, not of the values), turns them into (n, mean, M2, C) when it
// is done (qr_moments), and such records are combined pairwise with Chan et al.'s update
// (qr_combine_m) across lanes, waves, workgroups and parts of a field.  No division per element;
// the sums of products are explicit fused multiply-adds (one rounding, the same on host and device).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "cusz_amd.h"

#if defined(__HIPCC__)
#define QR_HD __host__ __device__
#else
#define QR_HD
#endif

namespace cusz_amd {

// ---- the partition: a fixed function of the length and the element size ---------------------
// A lane takes kQrVecs 16-byte vectors of consecutive elements per trip (an item); items go round
// the grid's lanes; the elements past the last whole item go one each to the first lanes.
constexpr int kQrBlock = 256;     // lanes per workgroup
constexpr int kQrWave = 64;
constexpr int kQrVecBytes = 16;
constexpr int kQrVecs = 2;
constexpr int kQrGridCap = 2048;  // workgroups (8 per CU on 256 CUs)
constexpr int kQrFinalBlock = 256;  // lanes of the one workgroup that combines the workgroups' records
constexpr uint64_t kQrNone = ~(uint64_t)0;

constexpr int qr_vec_elems(int elem_bytes) { return kQrVecBytes / elem_bytes; }
constexpr int qr_item_elems(int elem_bytes) { return kQrVecs * kQrVecBytes / elem_bytes; }
inline uint32_t qr_grid(uint64_t len, int elem_bytes)
{
  const uint64_t items = len / (uint64_t)qr_item_elems(elem_bytes), g = (items + kQrBlock - 1) / kQrBlock;
  return (uint32_t)(g < 1 ? 1 : g > (uint64_t)kQrGridCap ? (uint64_t)kQrGridCap : g);
}
inline uint32_t qr_region_grid(uint64_t nrows)  // a workgroup walks box rows b, b + grid, ...
{
  return (uint32_t)(nrows < 1 ? 1 : nrows > (uint64_t)kQrGridCap ? (uint64_t)kQrGridCap : nrows);
}

// ---- records --------------------------------------------------------------------------------
struct QrShift {  // a lane's shifted sums over pairs (a, b)
  double Ka, Kb, Sa, Sb, Saa, Sbb, Sab;
  uint64_t n;
};
struct QrMoments {  // n pairs: means, sums of squared deviations, sum of deviation products
  uint64_t n;
  double ma, mb, M2a, M2b, C;
};
struct QrLane {  // what a lane carries through the element loop; a = original, b = reconstruction
  QrShift s;
  double omin, omax, xmin, xmax;
  double max_e, max_pw, sum_e2;  // max |x - o|, max |x - o| / |o| over o != 0 (-inf: none), sum of squares
  uint64_t max_e_idx, n_unb, first_unb, first_diff;
};
struct QrCore {  // a lane, wave, workgroup or field; everything but the indices and n_unb over finite pairs
  QrMoments m;
  double omin, omax, xmin, xmax;
  double max_e, max_pw, sum_e2;
  uint64_t max_e_idx, n_unb, first_unb, first_diff;
};
struct QrPart : QrCore {  // the record as stored; without PSZ_AMD_QUALITY_AUTOCOR only the core is written and read
  QrMoments a1, a2;       // (o[i], o[i + 1]), (o[i], o[i + 2])
};

QR_HD inline bool qr_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }
QR_HD inline bool qr_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }

QR_HD inline void qr_shift_init(QrShift& s) { s.Ka = s.Kb = s.Sa = s.Sb = s.Saa = s.Sbb = s.Sab = 0.0, s.n = 0; }

QR_HD inline void qr_shift_add(QrShift& s, double a, double b)
{
  if (s.n == 0) s.Ka = a, s.Kb = b;
  const double da = a - s.Ka, db = b - s.Kb;
  s.Sa += da;
  s.Sb += db;
  s.Saa = __builtin_fma(da, da, s.Saa);
  s.Sbb = __builtin_fma(db, db, s.Sbb);
  s.Sab = __builtin_fma(da, db, s.Sab);
  s.n++;
}

QR_HD inline QrMoments qr_moments(const QrShift& s)
{
  QrMoments m{0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (s.n == 0) return m;
  const double n = (double)s.n, da = s.Sa / n, db = s.Sb / n;
  m.n = s.n;
  m.ma = s.Ka + da;
  m.mb = s.Kb + db;
  m.M2a = s.Saa - s.Sa * da;
  m.M2b = s.Sbb - s.Sb * db;
  m.C = s.Sab - s.Sa * db;
  m.M2a = m.M2a < 0.0 ? 0.0 : m.M2a;
  m.M2b = m.M2b < 0.0 ? 0.0 : m.M2b;
  return m;
}

// Chan, Golub, LeVeque: the moments of the union of two disjoint sets
QR_HD inline void qr_combine_m(QrMoments& a, const QrMoments& b)
{
  if (b.n == 0) return;
  if (a.n == 0) {
    a = b;
    return;
  }
  const double na = (double)a.n, nb = (double)b.n, n = na + nb;
  const double da = b.ma - a.ma, db = b.mb - a.mb, w = na * nb / n, f = nb / n;
  a.M2a += b.M2a + da * da * w;
  a.M2b += b.M2b + db * db * w;
  a.C += b.C + da * db * w;
  a.ma += da * f;
  a.mb += db * f;
  a.n += b.n;
}

QR_HD inline void qr_lane_init(QrLane& L)
{
  qr_shift_init(L.s);
  L.omin = L.xmin = INFINITY;
  L.omax = L.xmax = -INFINITY;
  L.max_e = L.max_pw = -INFINITY;
  L.sum_e2 = 0.0;
  L.max_e_idx = L.first_unb = L.first_diff = kQrNone;
  L.n_unb = 0;
}

template <typename T>
QR_HD inline bool qr_same_bits(T a, T b)
{
  if (sizeof(T) == 4) {
    uint32_t u, v;
    __builtin_memcpy(&u, &a, 4), __builtin_memcpy(&v, &b, 4);
    return u == v;
  }
  uint64_t u, v;
  __builtin_memcpy(&u, &a, 8), __builtin_memcpy(&v, &b, 8);
  return u == v;
}

// One pair at index i.  A lane meets its indices in ascending order, so `>` and the first hit keep
// the lowest index.  thr = 1.001 eb, or +inf for eb == 0 (nothing counts as unbounded then).
template <typename T>
QR_HD inline void qr_lane_add(QrLane& L, T ov, T xv, uint64_t i, double thr)
{
  const bool differ = !qr_same_bits(ov, xv);
  if (differ && L.first_diff == kQrNone) L.first_diff = i;
  const double o = (double)ov, x = (double)xv;
  bool unb;
  if (qr_finite(o) && qr_finite(x)) {
    qr_shift_add(L.s, o, x);
    L.omin = o < L.omin ? o : L.omin;
    L.omax = o > L.omax ? o : L.omax;
    L.xmin = x < L.xmin ? x : L.xmin;
    L.xmax = x > L.xmax ? x : L.xmax;
    const double e = __builtin_fabs(x - o), ao = __builtin_fabs(o);
    L.sum_e2 = __builtin_fma(e, e, L.sum_e2);
    if (e > L.max_e) L.max_e = e, L.max_e_idx = i;
    // e / ao can exceed the running maximum r only if e >= fl(r ao): the division is rare
    if (ao != 0.0 && e >= L.max_pw * ao) {
      const double q = e / ao;
      L.max_pw = q > L.max_pw ? q : L.max_pw;
    }
    unb = e > thr;
  }
  else
    unb = differ && thr < INFINITY;
  if (unb) {
    L.n_unb++;
    if (L.first_unb == kQrNone) L.first_unb = i;
  }
}

// An item of I consecutive pairs from index base on: what I calls of qr_lane_add give, bit for bit.
// When the lane has its shift and every value is finite (nearly always), the counts, the indices
// and the extrema are kept per item: the extrema in the element type (exact), the largest error as
// a running maximum whose index, like the unbounded and the first differing element, is looked for
// only in the item that moves it.
template <typename T, int I>
QR_HD inline void qr_lane_add_item(QrLane& L, const T* ov, const T* xv, uint64_t base, double thr)
{
  int fast = L.s.n != 0;  // (no short-circuit: one branch per item, not per value)
  for (int k = 0; k < I; k++) fast &= (int)qr_finite(ov[k]) & (int)qr_finite(xv[k]);
  if (!fast) {
    for (int k = 0; k < I; k++) qr_lane_add(L, ov[k], xv[k], base + k, thr);
    return;
  }
  T omin = ov[0], omax = ov[0], xmin = xv[0], xmax = xv[0];
  double e[I], emax = 0.0;
  int differ = 0;
  for (int k = 0; k < I; k++) {
    const double o = (double)ov[k], x = (double)xv[k];
    const double da = o - L.s.Ka, db = x - L.s.Kb;
    L.s.Sa += da;
    L.s.Sb += db;
    L.s.Saa = __builtin_fma(da, da, L.s.Saa);
    L.s.Sbb = __builtin_fma(db, db, L.s.Sbb);
    L.s.Sab = __builtin_fma(da, db, L.s.Sab);
    omin = ov[k] < omin ? ov[k] : omin;
    omax = ov[k] > omax ? ov[k] : omax;
    xmin = xv[k] < xmin ? xv[k] : xmin;
    xmax = xv[k] > xmax ? xv[k] : xmax;
    e[k] = __builtin_fabs(x - o);
    L.sum_e2 = __builtin_fma(e[k], e[k], L.sum_e2);
    emax = e[k] > emax ? e[k] : emax;
    const double ao = __builtin_fabs(o);
    if (ao != 0.0 && e[k] >= L.max_pw * ao) {
      const double q = e[k] / ao;
      L.max_pw = q > L.max_pw ? q : L.max_pw;
    }
    differ |= (int)!qr_same_bits(ov[k], xv[k]);
  }
  L.s.n += I;
  L.omin = (double)omin < L.omin ? (double)omin : L.omin;
  L.omax = (double)omax > L.omax ? (double)omax : L.omax;
  L.xmin = (double)xmin < L.xmin ? (double)xmin : L.xmin;
  L.xmax = (double)xmax > L.xmax ? (double)xmax : L.xmax;
  if (emax > L.max_e) {
    int at = 0;
    for (int k = I - 1; k >= 0; k--) at = e[k] == emax ? k : at;
    L.max_e = emax, L.max_e_idx = base + at;
  }
  if (emax > thr) {
    for (int k = 0; k < I; k++)
      if (e[k] > thr) {
        L.n_unb++;
        if (L.first_unb == kQrNone) L.first_unb = base + k;
      }
  }
  if (differ && L.first_diff == kQrNone) {
    int at = 0;
    for (int k = I - 1; k >= 0; k--) at = !qr_same_bits(ov[k], xv[k]) ? k : at;
    L.first_diff = base + at;
  }
}

// a pair of the autocorrelation: o[i] and o[i + k], counted when both are finite; one shift for both
QR_HD inline void qr_lag_add(QrShift& s, double a, double b)
{
  if (qr_finite(a) && qr_finite(b)) {
    if (s.n == 0) s.Ka = s.Kb = a;
    const double da = a - s.Ka, db = b - s.Kb;
    s.Sa += da;
    s.Sb += db;
    s.Saa = __builtin_fma(da, da, s.Saa);
    s.Sbb = __builtin_fma(db, db, s.Sbb);
    s.Sab = __builtin_fma(da, db, s.Sab);
    s.n++;
  }
}

// The lag pairs of an item: w holds the item's I originals and the two after it (any value where
// base + k >= len).  What qr_lag_add gives pair by pair, bit for bit; when all are finite and both
// records run on one shift, the deviations are computed once per element.
template <typename T, int I>
QR_HD inline void qr_lag_add_item(QrShift& a1, QrShift& a2, const T* w, uint64_t base, uint64_t len)
{
  int fast = a1.n != 0 && a2.n != 0 && base + I + 2 <= len && a2.Ka == a1.Ka && a2.Kb == a1.Ka && a1.Kb == a1.Ka;
  for (int k = 0; k < I + 2; k++) fast &= (int)qr_finite(w[k]);
  if (!fast) {
    for (int k = 0; k < I; k++) {
      if (base + k + 1 < len) qr_lag_add(a1, (double)w[k], (double)w[k + 1]);
      if (base + k + 2 < len) qr_lag_add(a2, (double)w[k], (double)w[k + 2]);
    }
    return;
  }
  double d[I + 2];
  for (int k = 0; k < I + 2; k++) d[k] = (double)w[k] - a1.Ka;
  for (int k = 0; k < I; k++) {
    a1.Sa += d[k], a1.Sb += d[k + 1], a2.Sa += d[k], a2.Sb += d[k + 2];
    a1.Saa = __builtin_fma(d[k], d[k], a1.Saa), a1.Sbb = __builtin_fma(d[k + 1], d[k + 1], a1.Sbb);
    a2.Saa = __builtin_fma(d[k], d[k], a2.Saa), a2.Sbb = __builtin_fma(d[k + 2], d[k + 2], a2.Sbb);
    a1.Sab = __builtin_fma(d[k], d[k + 1], a1.Sab), a2.Sab = __builtin_fma(d[k], d[k + 2], a2.Sab);
  }
  a1.n += I, a2.n += I;
}

QR_HD inline void qr_moments_init(QrMoments& m) { m.n = 0, m.ma = m.mb = m.M2a = m.M2b = m.C = 0.0; }

QR_HD inline void qr_core_init(QrCore& p)
{
  qr_moments_init(p.m);
  p.omin = p.xmin = INFINITY;
  p.omax = p.xmax = -INFINITY;
  p.max_e = p.max_pw = -INFINITY;
  p.sum_e2 = 0.0;
  p.max_e_idx = p.first_unb = p.first_diff = kQrNone;
  p.n_unb = 0;
}

QR_HD inline void qr_part_init(QrPart& p)
{
  qr_core_init(p);
  qr_moments_init(p.a1);
  qr_moments_init(p.a2);
}

QR_HD inline void qr_lane_core(const QrLane& L, QrCore& p)
{
  p.m = qr_moments(L.s);
  p.omin = L.omin, p.omax = L.omax, p.xmin = L.xmin, p.xmax = L.xmax;
  p.max_e = L.max_e, p.max_pw = L.max_pw, p.sum_e2 = L.sum_e2;
  p.max_e_idx = L.max_e_idx, p.n_unb = L.n_unb, p.first_unb = L.first_unb, p.first_diff = L.first_diff;
}

QR_HD inline void qr_lane_part(const QrLane& L, const QrShift& a1, const QrShift& a2, QrPart& p)
{
  qr_lane_core(L, p);
  p.a1 = qr_moments(a1);
  p.a2 = qr_moments(a2);
}

// a <- a (+) b.  Sums add in this order; ties of the largest error go to the lowest index.
QR_HD inline void qr_combine(QrCore& a, const QrCore& b)
{
  qr_combine_m(a.m, b.m);
  a.omin = b.omin < a.omin ? b.omin : a.omin;
  a.omax = b.omax > a.omax ? b.omax : a.omax;
  a.xmin = b.xmin < a.xmin ? b.xmin : a.xmin;
  a.xmax = b.xmax > a.xmax ? b.xmax : a.xmax;
  if (b.max_e > a.max_e || (b.max_e == a.max_e && b.max_e_idx < a.max_e_idx)) a.max_e = b.max_e, a.max_e_idx = b.max_e_idx;
  a.max_pw = b.max_pw > a.max_pw ? b.max_pw : a.max_pw;
  a.sum_e2 += b.sum_e2;
  a.n_unb += b.n_unb;
  a.first_unb = b.first_unb < a.first_unb ? b.first_unb : a.first_unb;
  a.first_diff = b.first_diff < a.first_diff ? b.first_diff : a.first_diff;
}

QR_HD inline void qr_combine(QrPart& a, const QrPart& b)  // with the autocorrelation pairs
{
  qr_combine(static_cast<QrCore&>(a), static_cast<const QrCore&>(b));
  qr_combine_m(a.a1, b.a1);
  qr_combine_m(a.a2, b.a2);
}

// ---- host: record <-> psz_amd_quality -------------------------------------------------------
inline double qr_corr(const QrMoments& m)
{
  const double n = (double)m.n;
  return (m.C / n) / (std::sqrt(m.M2a / n) * std::sqrt(m.M2b / n));
}

// the struct of a field of len elements from its record (the definitions: include/cusz_amd.h)
inline void qr_to_quality(const QrPart& p, size_t len, double eb, bool autocor, psz_amd_quality* q)
{
  const double nan = std::nan("");
  psz_statistics& s = q->stat;
  const double n = (double)p.m.n;
  if (p.m.n == 0) {
    s.odata = s.xdata = psz_data_summary{nan, nan, nan, nan, nan};
    s.score_PSNR = s.score_MSE = s.score_NRMSE = s.score_coeff = nan;
    s.max_err_abs = s.max_err_rel = s.max_err_pwrrel = nan;
  }
  else {
    s.odata.min = p.omin, s.odata.max = p.omax, s.odata.rng = p.omax - p.omin;
    s.odata.avg = p.m.ma, s.odata.std = std::sqrt(p.m.M2a / n);
    s.xdata.min = p.xmin, s.xdata.max = p.xmax, s.xdata.rng = p.xmax - p.xmin;
    s.xdata.avg = p.m.mb, s.xdata.std = std::sqrt(p.m.M2b / n);
    s.score_MSE = p.sum_e2 / n;
    s.score_NRMSE = std::sqrt(s.score_MSE) / s.odata.rng;
    s.score_PSNR = 20.0 * std::log10(s.odata.rng) - 10.0 * std::log10(s.score_MSE);
    s.score_coeff = (p.m.C / n) / (s.odata.std * s.xdata.std);
    s.max_err_abs = p.max_e;
    s.max_err_rel = p.max_e / s.odata.rng;
    s.max_err_pwrrel = p.max_pw == -INFINITY ? nan : p.max_pw;
  }
  s.max_err_idx = (size_t)p.max_e_idx;
  s.autocor_lag_one = autocor && p.a1.n ? qr_corr(p.a1) : nan;
  s.autocor_lag_two = autocor && p.a2.n ? qr_corr(p.a2) : nan;
  s.user_eb = eb;
  s.len = len;
  q->n_finite = (size_t)p.m.n;
  q->n_nonfinite = len - (size_t)p.m.n;
  q->n_unbounded = (size_t)p.n_unb;
  q->first_unbounded_idx = (size_t)p.first_unb;
  q->first_diff_idx = (size_t)p.first_diff;
}

// the record of a part from its struct, indices moved by the part's element offset (the merge)
inline QrPart qr_from_quality(const psz_amd_quality& q, size_t offset)
{
  QrPart p;
  qr_part_init(p);
  const psz_statistics& s = q.stat;
  auto shifted = [offset](size_t i) { return i == SIZE_MAX ? kQrNone : (uint64_t)i + offset; };
  p.n_unb = q.n_unbounded;
  p.first_unb = shifted(q.first_unbounded_idx);
  p.first_diff = shifted(q.first_diff_idx);
  if (q.n_finite == 0) return p;
  const double n = (double)q.n_finite;
  p.m.n = q.n_finite;
  p.m.ma = s.odata.avg, p.m.mb = s.xdata.avg;
  p.m.M2a = s.odata.std * s.odata.std * n, p.m.M2b = s.xdata.std * s.xdata.std * n;
  p.m.C = s.score_coeff == s.score_coeff ? s.score_coeff * s.odata.std * s.xdata.std * n : 0.0;  // NaN: a zero std
  p.omin = s.odata.min, p.omax = s.odata.max, p.xmin = s.xdata.min, p.xmax = s.xdata.max;
  p.max_e = s.max_err_abs, p.max_e_idx = shifted(s.max_err_idx);
  p.max_pw = s.max_err_pwrrel == s.max_err_pwrrel ? s.max_err_pwrrel : -INFINITY;
  p.sum_e2 = s.score_MSE * n;
  return p;
}

}  // namespace cusz_amd
