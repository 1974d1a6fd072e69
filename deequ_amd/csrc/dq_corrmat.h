// dq_corrmat.h -- the correlation matrix (dq_corrmat_*, include/deequ_amd.h): what the gfx950 kernel
// (dq_corrmat.hip), the pair kernel (dq_pair.hip) and the host mirror (dq_diag_corrmat_host) share.
// Plain C++: it compiles for the host alone (tools/corrmat_check.cpp) and for the device.
//
// One copy of the formulas: CorrelationState.sum (corr_merge), the shifted sums -> state conversion
// (corr_from_sums, the end of dq_corr_kernel) and the cancellation guard (moments_cancel).
//
// The matrix path cuts the rows of a batch into slabs of kCorrmatSlabRows consecutive rows (slab s =
// rows [s * kCorrmatSlabRows, ...), whatever the launch grid; a short tail joins the last slab).  Per slab and column i the shift c_i
// is the column's first selected (valid, `where` TRUE) finite value of the slab; with d_i(r) = x_i(r)
// - c_i on selected rows and 0 elsewhere, v_i(r) = 1 on selected rows and 0 elsewhere, the slab's
// pairwise-complete sums of the pair (i, j) are
//     n = Σ v_i v_j,  Sx = Σ d_i v_j,  Sy = Σ v_i d_j,  Sxx = Σ d_i² v_j,  Syy = Σ v_i d_j²,  Sxy = Σ d_i d_j.
// A slab's sums become a state (corr_from_sums) that is merged into the running state of its row
// range (corr_fold_slab); a pair some slab of which cannot be answered this way is flagged instead
// and answered for the whole batch by the pair kernel (the host mirror: corrmat_pair_rescue) or,
// where a sum of finite values was not finite, by Spark's per-row update (corr_update_row).
#pragma once

#include <stdint.h>

#ifndef DQ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DQ_HD __host__ __device__
#else
#define DQ_HD
#endif
#endif

namespace dq {

// Running state CorrelationState(n, xAvg, yAvg, ck, xMk, yMk) of a Correlation task.
struct CorrAcc {
  double n, xavg, yavg, ck, xmk, ymk;
};

// CorrelationState.sum (Correlation.scala:37-52); empty sides are identities.
DQ_HD inline void corr_merge(CorrAcc& a, const CorrAcc& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) {
    a = b;
    return;
  }
  const double n1 = a.n, n2 = b.n, n = n1 + n2;
  const double dx = b.xavg - a.xavg, dxn = dx / n;
  const double dy = b.yavg - a.yavg, dyn = dy / n;
  a.xavg = a.xavg + dxn * n2;
  a.yavg = a.yavg + dyn * n2;
  a.ck = a.ck + b.ck + dx * dyn * n1 * n2;
  a.xmk = a.xmk + b.xmk + dx * dxn * n1 * n2;
  a.ymk = a.ymk + b.ymk + dy * dyn * n1 * n2;
  a.n = n;
}

// Sums of n > 0 pairs about the shift (cx, cy) -> their state.
DQ_HD inline CorrAcc corr_from_sums(double cx, double cy, double n, double s_x, double s_y, double s_xx,
                                    double s_yy, double s_xy) {
  CorrAcc a;
  a.n = n;
  a.xavg = cx + s_x / n;
  a.yavg = cy + s_y / n;
  a.ck = s_xy - s_x * s_y / n;
  a.xmk = s_xx - s_x * s_x / n;
  a.ymk = s_yy - s_y * s_y / n;
  a.xmk = a.xmk < 0.0 ? 0.0 : a.xmk;  // rounding; NaN/Inf propagate
  a.ymk = a.ymk < 0.0 ? 0.0 : a.ymk;
  return a;
}

// Cancellation guard of the shifted moments.  Both value scans take a wave's Σd, Σd² about a
// shift c (a value of the column the wave saw first) and form m2 = S2 - S1²/n, whose relative
// rounding is about eps * S2 / m2: harmless while c lies near the data, but when c is an outlier
// (a 1e8 sentinel among N(0, 1) values) S1²/n is nearly all of S2 and the difference cancels.
// Spark's per-row update has no such mode (CentralMomentAgg, StandardDeviation.scala:37-44
// merge), so a wave whose S1²/n exceeds kMomentCancel * m2 makes its workgroup redo the moments
// of its chunk about the chunk's mean (then S1 ~ 0 and S2 ~ m2).  Ordinary data never comes close:
// a uniform column gives at most 3, a normal one needs c beyond 4 sigma.
constexpr double kMomentCancel = 16.0;
DQ_HD inline bool moments_cancel(double n, double S1, double S2) {
  const double q = S1 * S1 / n;
  return q > kMomentCancel * (S2 - q);  // (NaN / Inf moments: false, nothing to rescue)
}

// ---------------------------------------------------------------- the matrix path
constexpr int kCorrmatMaxCols = 64;        // columns of one matrix (4 x 4 tiles of 16 x 16)
constexpr int kCorrmatSlabRows = 1024;     // rows whose raw sums one accumulator holds
constexpr int kCorrmatChunkRows = 64;      // rows staged in LDS at a time (one validity word)

DQ_HD inline bool corrmat_finite(double x) { return x - x == 0.0; }

// Pairs (i, j), i <= j < k, in row-major order of the upper triangle.
DQ_HD inline int64_t corrmat_pair_index(int i, int j, int k) {
  return (int64_t)i * k - (int64_t)i * (i - 1) / 2 + (j - i);
}
DQ_HD inline int64_t corrmat_pairs(int k) { return (int64_t)k * (k + 1) / 2; }

// Why a slab's sums do not answer a pair (flag bits of a pair-batch).
constexpr uint32_t kCorrmatCancel = 1u;     // the shift was an outlier on either side (moments_cancel)
constexpr uint32_t kCorrmatNonFinite = 2u;  // a sum is not finite

// One slab's sums of the pair (i, j) about (cx, cy), folded into the running state of the slab's
// row range.  Not 0 (and `run` as it was): the pair is not answered from these sums -- one of them
// is not finite (kCorrmatNonFinite), or the shift was an outlier on either side (kCorrmatCancel; with
// n = 1 both moments are exactly 0 after the subtraction, so there is nothing to cancel).  diag:
// i == j, whose three moments (and two means) come from the one sum of squares (and the one sum).
DQ_HD inline uint32_t corr_fold_slab(CorrAcc& run, double cx, double cy, double n, double s_x, double s_y, double s_xx,
                                     double s_yy, double s_xy, bool diag) {
  if (n == 0.0) return 0u;
  if (diag) {
    s_y = s_x;
    s_yy = s_xy = s_xx;
  }
  if (!(corrmat_finite(s_x) && corrmat_finite(s_y) && corrmat_finite(s_xx) && corrmat_finite(s_yy) &&
        corrmat_finite(s_xy)))
    return kCorrmatNonFinite;
  if (n > 1.0 && (moments_cancel(n, s_x, s_xx) || moments_cancel(n, s_y, s_yy))) return kCorrmatCancel;
  CorrAcc a = corr_from_sums(cx, cy, n, s_x, s_y, s_xx, s_yy, s_xy);
  if (diag) a.ck = a.xmk;  // (the clamp at 0 included)
  corr_merge(run, a);
  return 0u;
}

// Spark's per-row Corr update (catalyst/StatefulCorrelation.scala:24-49) of one selected pair.  It
// forms no difference of two large sums, so finite values whose squared deviations overflow end as
// xMk = +Inf (the metric 0, as Spark's), where Sxx - Sx² / n would be Inf - Inf.  The rows of a pair
// whose sums were not finite are taken this way, a lane's rows at a time, and merged with corr_merge:
// Spark's own result for that partitioning of the rows.
DQ_HD inline void corr_update_row(CorrAcc& a, double x, double y) {
  const double n = a.n + 1.0;
  const double dx = x - a.xavg, dy = y - a.yavg;
  const double xavg = a.xavg + dx / n, yavg = a.yavg + dy / n;
  a.ck = a.ck + dx * (y - yavg);
  a.xmk = a.xmk + dx * (x - xavg);
  a.ymk = a.ymk + dy * (y - yavg);
  a.xavg = xavg;
  a.yavg = yavg;
  a.n = n;
}

// Slabs of a batch of n_rows rows: a tail shorter than half a slab belongs to the slab before it (a
// slab of a handful of rows has pairs of two or three rows, whose moments say nothing about the
// shift: the guard would send them to the pair kernel for no reason), so every slab but a batch's
// only one has 512 to 1535 rows.  Slab s = rows [s * kCorrmatSlabRows, corrmat_slab_end(s, ...)).
DQ_HD inline int64_t corrmat_n_slabs(int64_t n_rows) {
  const int64_t s = (n_rows + kCorrmatSlabRows / 2) / kCorrmatSlabRows;
  return n_rows > 0 && s < 1 ? 1 : s;
}
DQ_HD inline int64_t corrmat_slab_end(int64_t s, int64_t n_slabs, int64_t n_rows) {
  return s + 1 >= n_slabs ? n_rows : (s + 1) * kCorrmatSlabRows;
}

// Slabs per row range when n_slabs slabs are spread over at most max_ranges ranges (< 1: a range
// per slab).
DQ_HD inline int64_t corrmat_slabs_per_range(int64_t n_slabs, int64_t max_ranges) {
  return max_ranges < 1 ? 1 : (n_slabs + max_ranges - 1) / max_ranges;
}

// The fixed tree over a pair's row-range states (dq_corr_reduce_kernel's, for `width` leaves slots):
// slot t merges ranges [t * per, (t + 1) * per) in order, then slot t takes slot t + s for s = 1, 2, 4...
template <typename Get>
inline CorrAcc corrmat_tree_host(int64_t n_ranges, int width, const Get& get) {
  const int64_t per = (n_ranges + width - 1) / width;
  CorrAcc* slot = new CorrAcc[width];
  for (int t = 0; t < width; ++t) {
    CorrAcc a{0, 0, 0, 0, 0, 0};
    for (int64_t b = (int64_t)t * per; b < (int64_t)(t + 1) * per && b < n_ranges; ++b) corr_merge(a, get(b));
    slot[t] = a;
  }
  for (int s = 1; s < width; s <<= 1)
    for (int t = 0; t + s < width; t += 2 * s) corr_merge(slot[t], slot[t + s]);
  const CorrAcc r = slot[0];
  delete[] slot;
  return r;
}

// The pair kernel's answer on the host, for the pairs the matrix sums do not answer: per slab the
// sums about the slab's own means (two passes), merged in slab order.
inline CorrAcc corrmat_pair_rescue(const double* x, const uint8_t* vx, const double* y, const uint8_t* vy,
                                   const uint8_t* where, int64_t n_rows) {
  CorrAcc run{0, 0, 0, 0, 0, 0};
  for (int64_t r0 = 0; r0 < n_rows; r0 += kCorrmatSlabRows) {
    const int64_t r1 = r0 + kCorrmatSlabRows < n_rows ? r0 + kCorrmatSlabRows : n_rows;
    auto sel = [&](int64_t r) { return (!vx || vx[r]) && (!vy || vy[r]) && (!where || where[r]); };
    double n = 0, mx = 0, my = 0;
    for (int64_t r = r0; r < r1; ++r)
      if (sel(r)) {
        n += 1.0;
        mx += x[r];
        my += y[r];
      }
    if (n == 0.0) continue;
    mx /= n;
    my /= n;
    double s_x = 0, s_y = 0, s_xx = 0, s_yy = 0, s_xy = 0;
    for (int64_t r = r0; r < r1; ++r)
      if (sel(r)) {
        const double dx = x[r] - mx, dy = y[r] - my;
        s_x += dx;
        s_y += dy;
        s_xx += dx * dx;
        s_yy += dy * dy;
        s_xy += dx * dy;
      }
    corr_merge(run, corr_from_sums(mx, my, n, s_x, s_y, s_xx, s_yy, s_xy));
  }
  return run;
}

// ... and of the pairs whose sums were not finite: Spark's per-row update over the batch's rows.
inline CorrAcc corrmat_pair_rows(const double* x, const uint8_t* vx, const double* y, const uint8_t* vy,
                                 const uint8_t* where, int64_t n_rows) {
  CorrAcc run{0, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < n_rows; ++r)
    if ((!vx || vx[r]) && (!vy || vy[r]) && (!where || where[r])) corr_update_row(run, x[r], y[r]);
  return run;
}

// The host mirror of one batch: columns of doubles (the values already cast), a byte per row for
// each column's validity (nullptr: no NULLs) and for the `where` (nullptr: none).  states: 6 doubles
// per pair (six zeros: no row has both); flags[p] = 1 where pair p was not answered from the matrix
// sums.  The same slabs, shifts, guard, flags and merge order as the kernel, over at most
// max_ranges row ranges; the sums themselves are plain loops in row order.
inline void corrmat_host(const double* const* cols, const uint8_t* const* valid, const uint8_t* where, int k,
                         int64_t n_rows, int64_t max_ranges, double* states, uint8_t* flags) {
  const int64_t n_pairs = corrmat_pairs(k);
  const int64_t n_slabs = corrmat_n_slabs(n_rows);
  const int64_t per = n_slabs > 0 ? corrmat_slabs_per_range(n_slabs, max_ranges) : 1;
  const int64_t n_ranges = n_slabs > 0 ? (n_slabs + per - 1) / per : 0;
  CorrAcc* part = new CorrAcc[(size_t)(n_pairs * (n_ranges > 0 ? n_ranges : 1))];
  uint8_t* col_bad = new uint8_t[(size_t)k];
  double* shift = new double[(size_t)k];
  constexpr int64_t kStride = 2 * kCorrmatSlabRows;  // (a slab holds at most 1.5 kCorrmatSlabRows rows)
  double* d = new double[(size_t)k * kStride];
  uint8_t* v = new uint8_t[(size_t)k * kStride];
  for (int64_t p = 0; p < n_pairs; ++p) flags[p] = 0;
  for (int i = 0; i < k; ++i) col_bad[i] = 0;
  for (int64_t g = 0; g < n_ranges; ++g) {
    for (int64_t p = 0; p < n_pairs; ++p) part[p * n_ranges + g] = CorrAcc{0, 0, 0, 0, 0, 0};
    for (int64_t s = g * per; s < (g + 1) * per && s < n_slabs; ++s) {
      const int64_t r0 = s * kCorrmatSlabRows;
      const int64_t rows = corrmat_slab_end(s, n_slabs, n_rows) - r0;
      for (int i = 0; i < k; ++i) {
        bool have = false;
        shift[i] = 0.0;
        for (int64_t r = 0; r < rows; ++r) {
          const int64_t row = r0 + r;
          const bool sel = (!valid || !valid[i] || valid[i][row]) && (!where || where[row]);
          const double x = cols[i][row];
          const bool fin = corrmat_finite(x);
          if (sel && !fin) col_bad[i] = 1;
          if (sel && fin && !have) {
            have = true;
            shift[i] = x;
          }
          v[(size_t)i * kStride + r] = sel ? 1 : 0;
          d[(size_t)i * kStride + r] = sel && fin ? x - shift[i] : 0.0;
        }
      }
      for (int i = 0; i < k; ++i)
        for (int j = i; j < k; ++j) {
          const double* di = d + (size_t)i * kStride;
          const double* dj = d + (size_t)j * kStride;
          const uint8_t* vi = v + (size_t)i * kStride;
          const uint8_t* vj = v + (size_t)j * kStride;
          double n = 0, s_x = 0, s_y = 0, s_xx = 0, s_yy = 0, s_xy = 0;
          for (int64_t r = 0; r < rows; ++r) {
            const double a = vi[r], b = vj[r];
            n += a * b;
            s_x += di[r] * b;
            s_y += a * dj[r];
            s_xx += di[r] * di[r] * b;
            s_yy += a * (dj[r] * dj[r]);
            s_xy += di[r] * dj[r];
          }
          const int64_t p = corrmat_pair_index(i, j, k);
          flags[p] |= (uint8_t)corr_fold_slab(part[p * n_ranges + g], shift[i], shift[j], n, s_x, s_y, s_xx, s_yy, s_xy,
                                              i == j);
        }
    }
  }
  for (int i = 0; i < k; ++i)
    for (int j = i; j < k; ++j) {
      const int64_t p = corrmat_pair_index(i, j, k);
      const bool bad = col_bad[i] || col_bad[j];
      CorrAcc a;
      if (!bad && (flags[p] & kCorrmatNonFinite))
        a = corrmat_pair_rows(cols[i], valid ? valid[i] : nullptr, cols[j], valid ? valid[j] : nullptr, where, n_rows);
      else if (bad || flags[p])
        a = corrmat_pair_rescue(cols[i], valid ? valid[i] : nullptr, cols[j], valid ? valid[j] : nullptr, where, n_rows);
      else
        a = corrmat_tree_host(n_ranges, 256, [&](int64_t b) { return part[p * n_ranges + b]; });
      flags[p] = bad || flags[p] ? 1 : 0;
      double* o = states + 6 * p;
      o[0] = a.n, o[1] = a.xavg, o[2] = a.yavg, o[3] = a.ck, o[4] = a.xmk, o[5] = a.ymk;
      if (a.n == 0.0) o[1] = o[2] = o[3] = o[4] = o[5] = 0.0;
    }
  delete[] part;
  delete[] col_bad;
  delete[] shift;
  delete[] d;
  delete[] v;
}

}  // namespace dq
