// eval_host_fuzz.cpp -- the scoring arithmetic (codenet_amd/csrc/cdn_eval.h: the append with its two-decimal cut, the
// sort key, the rank, the COCO matcher, the VOC argmax / bookkeeping, numpy's pairwise sum -- the text the GPU kernels
// run) on random tables, on the host, under AddressSanitizer and UndefinedBehaviorSanitizer.  Plain C++ with its own
// main; no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o build/eval_host_fuzz tools/probes/eval_host_fuzz.cpp
//   build/eval_host_fuzz [rounds = 2000]
//
// Per round: a random merge block (row counts inside and outside [0, R], NaN / Inf / huge / negative numbers among the
// boxes and scores) appended to a table smaller than the block, so that the overflow path runs; keys, and the header's
// ranked list of every class (rank_rows over a poisoned buffer: with NaN scores it must still be a permutation of the
// class's rows); random ground truths (zero-area, crowd, G = 0); the 40 COCO matchers with and without a
// precomputed IoU matrix, whose flags must agree; the VOC argmax; a pairwise sum against its recursive definition.  Every
// buffer is a heap block of exactly the size the header is told, with 64 guard bytes on either side that must stay intact.
// What it does not reach: the loops over images and classes of the cdn_eval_*_host entries and the accumulate passes,
// which live in codenet_eval.hip beside the kernels; tests/test_eval_device_host.py runs those.
// Exit status 0: every call returned, no guard byte changed and the paired results agreed; the sanitizers abort otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codenet_amd/csrc/cdn_eval.h"

namespace E = cdn_eval;

namespace {

constexpr int kGuard = 64;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)(s >> 32);
  }
  int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
  double unit() { return next() / 4294967296.0; }
};

template <typename T>
struct Guarded {                     // n elements between two guard zones
  std::vector<unsigned char> raw;
  size_t n;
  explicit Guarded(size_t count) : raw(2 * kGuard + count * sizeof(T) + 1, 0xA5), n(count) {
    for (size_t i = 0; i < count * sizeof(T); ++i) raw[kGuard + i] = 0;
  }
  T *data() { return reinterpret_cast<T *>(raw.data() + kGuard); }
  bool intact() const {
    for (int i = 0; i < kGuard; ++i)
      if (raw[i] != 0xA5 || raw[kGuard + n * sizeof(T) + i] != 0xA5) return false;
    return true;
  }
};

float wild(Rng &r) {
  switch (r.below(12)) {
    case 0: return NAN;
    case 1: return INFINITY;
    case 2: return -INFINITY;
    case 3: return 3.0e38f;
    case 4: return -1.0e30f;
    case 5: return -0.0f;
    default: return (float)(r.unit() * 600.0 - 50.0);
  }
}

double recursive_sum(const double *a, int64_t n) {      // numpy's definition, as written
  if (n <= 128) return E::np_block_sum(a, n);
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return recursive_sum(a, n2) + recursive_sum(a + n2, n - n2);
}

int fail(const char *what, int round) {
  std::fprintf(stderr, "eval_host_fuzz: %s (round %d)\n", what, round);
  return 1;
}

int one_round(Rng &r, int round) {
  const int classes = 1 + r.below(6), R = 1 + r.below(40), cap = 1 + r.below(48), coco = r.below(2);
  Guarded<float> boxes((size_t)classes * R * 5);
  Guarded<int> rows(classes), pre(classes + 1);
  Guarded<double> det((size_t)cap * E::kCols);
  for (size_t i = 0; i < boxes.n; ++i) boxes.data()[i] = r.below(4) ? (float)(r.below(200)) : wild(r);
  int acc = 0;
  for (int c = 0; c < classes; ++c) {
    rows.data()[c] = r.below(10) ? r.below(R + 1) : (r.below(2) ? -5 : R + 1000);
    pre.data()[c] = acc;
    acc += E::clamp_rows(rows.data()[c], R);
  }
  pre.data()[classes] = acc;
  const int base = r.below(cap + 1);
  for (int k = 0; k < base; ++k) {
    for (int j = 0; j < 5; ++j) det.data()[k * E::kCols + j] = (double)r.below(100);
    det.data()[k * E::kCols + 5] = (double)r.below(classes);
  }
  const int nth = 1 + r.below(4);
  for (int tid = 0; tid < nth; ++tid)
    E::append_image(boxes.data(), pre.data(), 0, classes, R, det.data(), base, cap, coco, tid, nth);
  const int n = base + acc > cap ? cap : base + acc;
  if (!boxes.intact() || !rows.intact() || !pre.intact() || !det.intact()) return fail("guard bytes changed by append", round);
  // keys, ranks
  Guarded<int64_t> keys(cap);
  for (int i = 0; i < cap; ++i) {
    int bad = 0;
    keys.data()[i] = E::sort_key(det.data() + (size_t)i * E::kCols, i < n, classes, coco, &bad);
    const int64_t cls = keys.data()[i] >> 32;
    if (cls < 0 || cls > classes) return fail("key class out of range", round);
  }
  Guarded<int> order(E::kMaxDet), rank(cap);
  Guarded<unsigned char> dtm(cap), dtig(cap), dtm2(cap), dtig2(cap);
  for (int cls = 0; cls < classes; ++cls) {
    // the header's own ranked list over a poisoned buffer: every slot below D must have been written with a row of the table
    for (int k = 0; k < E::kMaxDet; ++k) order.data()[k] = 0x7fffffff;
    const int D = E::rank_rows(det.data(), n, cls, E::kMaxDet, order.data(), rank.data());
    for (int d = 0; d < D; ++d) {
      const int row = order.data()[d];
      if (row < 0 || row >= n || rank.data()[row] != d || (int)det.data()[(size_t)row * E::kCols + 5] != cls)
        return fail("ranked list is not a permutation of the class's rows", round);
    }
    const int G = r.below(4) ? r.below(20) : 0;
    Guarded<double> gt((size_t)G * 4), area(G), iou((size_t)D * G);
    Guarded<int> flag(G);
    Guarded<unsigned char> gtm(G), seen(G);
    for (int g = 0; g < G; ++g) {
      for (int j = 0; j < 4; ++j) gt.data()[g * 4 + j] = r.below(8) ? (double)r.below(200) : (double)wild(r);
      area.data()[g] = r.below(6) ? (double)r.below(20000) : 0.0;
      flag.data()[g] = r.below(5) == 0;
    }
    E::CocoImg c{det.data(), order.data(), D, gt.data(), area.data(), flag.data(), G, nullptr};
    for (int k = 0; k < D * G; ++k) iou.data()[k] = E::coco_iou_at(c, k / G, k % G);
    E::CocoImg cm = c;
    cm.iou = iou.data();
    const double lo = r.below(2) ? 0.0 : 1024.0, hi = r.below(2) ? 1e10 : 9216.0, thr = 0.5 + 0.05 * r.below(10);
    const int n1 = E::coco_match_lane(c, thr, lo, hi, gtm.data(), dtm.data(), dtig.data());
    const int n2 = E::coco_match_lane(cm, thr, lo, hi, gtm.data(), dtm2.data(), dtig2.data());
    if (n1 != n2) return fail("non-ignored counts differ", round);
    for (int d = 0; d < D; ++d) {
      const int row = order.data()[d];
      if (dtm.data()[row] != dtm2.data()[row] || dtig.data()[row] != dtig2.data()[row]) return fail("matrix and on-the-fly flags differ", round);
    }
    // VOC argmax + bookkeeping over the same boxes
    for (int d = 0; d < D; ++d) {
      double best = 0.0;
      int bidx = -1;
      for (int g = 0; g < G; ++g) {
        const double ov = E::voc_overlap(det.data() + (size_t)order.data()[d] * E::kCols, gt.data() + g * 4);
        if (E::voc_better(ov, g, best, bidx)) {
          best = ov;
          bidx = g;
        }
      }
      unsigned char tp, fp;
      E::voc_classify(best, bidx, 0.5, flag.data(), seen.data(), &tp, &fp);
      if (tp && fp) return fail("TP and FP at once", round);
    }
    if (!gt.intact() || !area.intact() || !iou.intact() || !flag.intact() || !gtm.intact() || !seen.intact())
      return fail("guard bytes changed by a matcher", round);
  }
  if (!keys.intact() || !order.intact() || !rank.intact() || !dtm.intact() || !dtig.intact() || !dtm2.intact() || !dtig2.intact() ||
      !det.intact())
    return fail("guard bytes changed", round);
  // the pairwise sum against its recursive definition, lengths on both sides of the block and split sizes
  const int64_t len = r.below(3) ? r.below(300) : r.below(5000);
  Guarded<double> terms(len);
  for (int64_t i = 0; i < len; ++i) terms.data()[i] = r.unit() - 0.3;
  if (E::np_pairwise_sum(terms.data(), len) != recursive_sum(terms.data(), len)) return fail("pairwise sum differs", round);
  return terms.intact() ? 0 : fail("guard bytes changed by the sum", round);
}

}  // namespace

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
  Rng r{0x9E3779B97F4A7C15ull};
  for (int i = 0; i < rounds; ++i)
    if (one_round(r, i)) return 1;
  std::printf("eval_host_fuzz: %d rounds ok\n", rounds);
  return 0;
}
