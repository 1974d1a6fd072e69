// dq_kll.cpp -- the host side of KLLSketch: the reference's sequential sketch restated
// (QuantileNonSample.scala:72-112, :215-230; NonSampleCompactor.scala:38-68), the capacity table
// and the rank queries.  The library merges the batches' sketches with it; dq_diag_kll_sketch and
// tools/kll_check.cpp run the whole slab-and-tree layout with it on the CPU.  No HIP here.
#include "dq_kll.h"

#include <algorithm>
#include <cmath>

namespace dq {
namespace kll {

int64_t capacity(int32_t sketch_size, double shrinking_factor, int height) {
  const double x = std::ceil((double)sketch_size * std::pow(shrinking_factor, (double)height) / 2);
  int64_t i;  // Double.toInt: NaN -> 0, saturating
  if (x != x) i = 0;
  else if (x >= 2147483647.0) i = 2147483647;
  else if (x <= -2147483648.0) i = -2147483647 - 1;
  else i = (int64_t)x;
  return (int64_t)(int32_t)(uint32_t)(2u * (uint32_t)(i + 1));  // Int arithmetic wraps
}

void capacity_table(int32_t sketch_size, double shrinking_factor, int32_t* cap, int64_t* sum) {
  int64_t s = 0;
  for (int h = 0; h < kMaxLevels; ++h) {
    cap[h] = (int32_t)capacity(sketch_size, shrinking_factor, h);
    s += cap[h] > 0 ? cap[h] : 0;
  }
  if (sum) *sum = s;
}

int levels_bound(const int32_t* cap, int64_t n) {
  // level H-1 is created by a compaction of level H-2, which then held at least cap[H-2] items
  // of weight 2^(H-2) each
  int H = 1;
  while (H < kMaxLevels) {
    const int h = H - 1;  // the level whose compaction would create level H
    if (h >= 62 || (int64_t)cap[h] > (n >> h)) break;
    ++H;
  }
  return H;
}

static uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

bool java_less(double a, double b) {
  if (a < b) return true;
  if (a > b) return false;
  // equal, or a NaN: compare doubleToLongBits (NaNs collapsed) as signed longs
  const int64_t x = a != a ? 0x7ff8000000000000ll : (int64_t)bits(a);
  const int64_t y = b != b ? 0x7ff8000000000000ll : (int64_t)bits(b);
  return x < y;
}

double java_min(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && (bits(b) >> 63)) return b;
  return a <= b ? a : b;  // (b NaN: a <= b is false, b returned)
}

double java_max(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && (bits(a) >> 63)) return b;
  return a >= b ? a : b;
}

std::vector<double> Compactor::compact() {
  const size_t items = buf.size();
  const size_t len = items - (items % 2);
  if (num_compress % 2 == 1) offset = 1 - offset;
  std::vector<double> sorted(buf.begin(), buf.begin() + len);
  std::stable_sort(sorted.begin(), sorted.end(), java_less);
  std::vector<double> out;
  out.reserve(len / 2);
  for (size_t i = (size_t)offset; i < len; i += 2) out.push_back(sorted[i]);
  std::vector<double> rest;
  if (items % 2 == 1) rest.push_back(buf[items - 1]);  // the odd tail is the last appended item
  buf.swap(rest);
  ++num_compress;
  return out;
}

Sketch::Sketch(int32_t k, double c) : sketch_size(k), shrinking_factor(c) { expand(); }

void Sketch::expand() {
  levels.emplace_back();
  total = 0;
  for (size_t h = 0; h < levels.size(); ++h) total += cap((int)h);
}

void Sketch::update(double v) {
  levels[0].buf.push_back(v);
  ++actual;
  if (actual > total) condense();
}

void Sketch::update_untyped(double v) {
  min = java_min(min, v);
  max = java_max(max, v);
  update(v);
}

void Sketch::condense() {
  for (size_t h = 0; h < levels.size(); ++h) {
    if ((int64_t)levels[h].buf.size() >= cap((int)h)) {
      if (h + 1 >= levels.size()) expand();
      const std::vector<double> out = levels[h].compact();
      levels[h + 1].buf.insert(levels[h + 1].buf.end(), out.begin(), out.end());
      actual = 0;
      for (const Compactor& c : levels) actual += (int64_t)c.buf.size();
      break;
    }
  }
}

void Sketch::merge(const Sketch& that) {
  while (levels.size() < that.levels.size()) expand();
  for (size_t i = 0; i < that.levels.size(); ++i)
    levels[i].buf.insert(levels[i].buf.end(), that.levels[i].buf.begin(), that.levels[i].buf.end());
  actual = 0;
  for (const Compactor& c : levels) actual += (int64_t)c.buf.size();
  while (actual >= total) {
    const int64_t before = actual;
    const size_t lv = levels.size();
    condense();
    if (actual == before && levels.size() == lv) break;  // (no level at capacity: the reference would spin)
  }
}

void Sketch::merge_untyped(const Sketch& that) {
  min = java_min(min, that.min);
  max = java_max(max, that.max);
  merge(that);
}

int64_t Sketch::rank(double x) const {  // Ordering.Double.gt is the primitive `>`
  int64_t r = 0;
  for (size_t h = 0; h < levels.size(); ++h)
    for (double t : levels[h].buf)
      if (!(t > x)) r += (int64_t)1 << h;
  return r;
}

int64_t Sketch::rank_exclusive(double x) const {
  int64_t r = 0;
  for (size_t h = 0; h < levels.size(); ++h)
    for (double t : levels[h].buf)
      if (t < x) r += (int64_t)1 << h;
  return r;
}

int64_t Sketch::weight() const {
  int64_t w = 0;
  for (size_t h = 0; h < levels.size(); ++h) w += (int64_t)levels[h].buf.size() << h;
  return w;
}

int64_t Sketch::export_words() const {
  int64_t n = 3 + 3 * (int64_t)levels.size();
  for (const Compactor& c : levels) n += (int64_t)c.buf.size();
  return n;
}

void Sketch::export_to(void* out) const {
  // 8-byte words: int64 n_levels, double min, double max, per level {int64 length, numOfCompress,
  // offset}, then the items level by level
  uint8_t* p = static_cast<uint8_t*>(out);
  auto put_i = [&p](int64_t v) { memcpy(p, &v, 8); p += 8; };
  auto put_d = [&p](double v) { memcpy(p, &v, 8); p += 8; };
  put_i((int64_t)levels.size());
  put_d(min);
  put_d(max);
  for (const Compactor& c : levels) {
    put_i((int64_t)c.buf.size());
    put_i(c.num_compress);
    put_i(c.offset);
  }
  for (const Compactor& c : levels)
    for (double v : c.buf) put_d(v);
}

Sketch sketch_slabs(const double* values, const uint8_t* valid, int64_t n, int32_t k, double c, int64_t slab_rows) {
  std::vector<Sketch> slabs;
  for (int64_t r0 = 0; r0 < n; r0 += slab_rows) {
    slabs.emplace_back(k, c);
    Sketch& s = slabs.back();
    const int64_t r1 = std::min(n, r0 + slab_rows);
    for (int64_t r = r0; r < r1; ++r)
      if (!valid || valid[r]) s.update_untyped(values[r]);
  }
  if (slabs.empty()) return Sketch(k, c);
  for (size_t step = 1; step < slabs.size(); step *= 2)
    for (size_t j = 0; j + step < slabs.size(); j += 2 * step) slabs[j].merge_untyped(slabs[j + step]);
  return std::move(slabs[0]);
}

}  // namespace kll
}  // namespace dq
