// dq_quantile.cpp -- the host side of ApproxQuantile's digest (dq_quantile.h; DESIGN.md,
// ApproxQuantile): the batch summary from the keys the select found, the Greenwald-Khanna merge and
// compress, the query, and the serialised form.  Plain C++: tools/aq_check.cpp runs it under the
// host sanitizers.
#include "dq_quantile.h"

#include <algorithm>
#include <cmath>

namespace dq {
namespace aq {

Digest Digest::from_batch(double eps, int64_t n, const uint64_t* keys, int64_t m) {
  Digest d(eps);
  if (n <= 0 || m <= 0) return d;
  const int64_t gap = batch_gap(eps, n);
  d.count = n;
  d.sampled.resize((size_t)m);
  int64_t prev = 0;
  for (int64_t j = 0; j < m; ++j) {
    const int64_t r = batch_rank(j, m, n, gap);
    d.sampled[(size_t)j] = Entry{value_of_key(keys[j]), r - prev, 0};
    prev = r;
  }
  return d;
}

bool Digest::merge(const Digest& that) {
  if (that.eps != eps) return false;
  if (that.sampled.empty()) return true;
  if (sampled.empty()) {
    sampled = that.sampled;
    count = that.count;
    return true;
  }
  const std::vector<Entry>&A = sampled, &B = that.sampled;
  const size_t na = A.size(), nb = B.size();
  // merged order: by key, this side's entries before the other's on ties
  std::vector<Entry> all;
  std::vector<uint8_t> side;
  all.reserve(na + nb);
  side.reserve(na + nb);
  size_t i = 0, j = 0;
  while (i < na || j < nb) {
    const bool take_a = j == nb || (i < na && key_of_value(A[i].value) <= key_of_value(B[j].value));
    all.push_back(take_a ? A[i++] : B[j++]);
    side.push_back(take_a ? 0 : 1);
  }
  // delta grows by g + delta - 1 of the next entry of the other side (its values before the merge)
  const Entry* next[2] = {nullptr, nullptr};
  std::vector<int64_t> grown(all.size());
  for (size_t k = all.size(); k-- > 0;) {
    const Entry* s = next[1 - side[k]];
    grown[k] = all[k].delta + (s ? s->g + s->delta - 1 : 0);
    next[side[k]] = &all[k];
  }
  for (size_t k = 0; k < all.size(); ++k) all[k].delta = grown[k];
  count += that.count;
  // compress from the right; the first and the last entry stay
  const int64_t threshold = (int64_t)std::floor(2.0 * eps * (double)count);
  std::vector<Entry> kept;
  kept.reserve(all.size());
  Entry head = all.back();
  for (size_t k = all.size() - 1; k-- > 1;) {
    const Entry& e = all[k];
    if (e.g + head.g + head.delta <= threshold) {
      head.g += e.g;
    } else {
      kept.push_back(head);
      head = e;
    }
  }
  kept.push_back(head);
  if (all.size() > 1) kept.push_back(all.front());
  sampled.assign(kept.rbegin(), kept.rend());
  return true;
}

double Digest::query(double q, bool* empty) const {
  *empty = sampled.empty();
  if (sampled.empty()) return 0.0;
  const int64_t t = (int64_t)std::ceil(q * (double)count);
  int64_t rmin = 0, best = 0;
  size_t at = 0;
  for (size_t k = 0; k < sampled.size(); ++k) {
    rmin += sampled[k].g;
    const int64_t rmax = rmin + sampled[k].delta;
    const int64_t err = std::max(t - rmin, rmax - t);
    if (k == 0 || err < best) {
      best = err;
      at = k;
    }
  }
  return sampled[at].value;
}

bool Digest::fits_int32() const {
  for (const Entry& e : sampled)
    if (e.g > 0x7fffffff || e.delta > 0x7fffffff || e.g < 0 || e.delta < 0) return false;
  return sampled.size() <= 0x7fffffffu;
}

namespace {
void put_be(uint8_t*& p, uint64_t v, int bytes) {
  for (int k = bytes - 1; k >= 0; --k) *p++ = (uint8_t)(v >> (8 * k));
}
uint64_t get_be(const uint8_t*& p, int bytes) {
  uint64_t v = 0;
  for (int k = 0; k < bytes; ++k) v = (v << 8) | *p++;
  return v;
}
uint64_t double_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
double bits_double(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}
}  // namespace

void Digest::serialise(uint8_t* out) const {
  uint8_t* p = out;
  put_be(p, (uint32_t)kCompressThreshold, 4);
  put_be(p, double_bits(eps), 8);
  put_be(p, (uint64_t)count, 8);
  put_be(p, (uint32_t)sampled.size(), 4);
  for (const Entry& e : sampled) {
    put_be(p, double_bits(e.value), 8);
    put_be(p, (uint32_t)(int32_t)e.g, 4);
    put_be(p, (uint32_t)(int32_t)e.delta, 4);
  }
}

bool Digest::deserialise(const uint8_t* in, int64_t len, Digest* out) {
  if (len < 24) return false;
  const uint8_t* p = in;
  get_be(p, 4);
  Digest d(bits_double(get_be(p, 8)));
  d.count = (int64_t)get_be(p, 8);
  const int64_t n = (int32_t)(uint32_t)get_be(p, 4);
  if (n < 0 || len < 24 + 16 * n) return false;
  d.sampled.resize((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    Entry& e = d.sampled[(size_t)k];
    e.value = bits_double(get_be(p, 8));
    e.g = (int32_t)(uint32_t)get_be(p, 4);
    e.delta = (int32_t)(uint32_t)get_be(p, 4);
  }
  *out = d;
  return true;
}

}  // namespace aq
}  // namespace dq
