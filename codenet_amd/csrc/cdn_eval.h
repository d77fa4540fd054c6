// cdn_eval.h -- detection scoring: VOC07 AP and COCO bbox mAP (DESIGN.md section 7.4e is the contract; tests/coco_eval_ref.py
// restates the COCO half in numpy, tools/eval_voc.py::voc_eval_curve the VOC half).  Plain C++ with no HIP call: the
// two-decimal cut, the sort key, the two overlap formulas, the per-image rank, the sequential matchers and the element
// arithmetic of the accumulation.  Everything is __host__ __device__ under hipcc: the kernels of codenet_eval.hip and the
// cdn_eval_*_host entries run the SAME text -- the kernels with the lanes of a wave or the threads of a workgroup, the
// host with one lane.  tools/probes/eval_host_fuzz.cpp includes this file alone.
//
// All box arithmetic is float64 and every operation is rounded on its own (fp contract off): an FMA formed from
// `da + ga - w * h` would change bits.  Sums that cross lanes are integer counts or maxima, so no order can change a bit.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define CDN_EVAL_HD __host__ __device__ __forceinline__
#else
#define CDN_EVAL_HD inline
#endif
#if defined(__clang__)
#define CDN_EVAL_NOFMA _Pragma("clang fp contract(off)")
#else
#define CDN_EVAL_NOFMA
#endif

namespace cdn_eval {

constexpr int kCols = 6;                    // table row: x1 y1 x2 y2 score class (VOC) / x y w h score class (COCO)
constexpr int kThr = 10, kAreas = 4, kMaxDetsN = 3, kRec = 101;      // COCOeval's Params for bbox
constexpr int kLanes = kThr * kAreas;       // the independent sequential matchers of one (image, category)
constexpr int kMaxDet = 100;                // maxDets[-1]: what computeIoU and evaluateImg keep per (image, category)
constexpr int kMaxCap = 1024;               // rows per image the rank's LDS list holds
constexpr int kMaxClasses = 256;
constexpr int kLdsIou = 4096;               // doubles: the D x G matrix lives in LDS when it fits
enum Flag { kFlagOverflow = 1, kFlagScore = 2 };

CDN_EVAL_HD int max_dets(int m) { return m == 0 ? 1 : (m == 1 ? 10 : 100); }

// float("{:.2f}".format(v)) for a float32 v: v * 100 is exact in double (24 x 7 significand bits), rint ties to even on
// that exact value as the decimal formatting does, and the division is the correctly rounded quotient the parser returns
CDN_EVAL_HD double cut2(float v) {
  CDN_EVAL_NOFMA
  const double p = (double)v * 100.0;
  return rint(p) / 100.0;
}

// one row of the merge block -> one table row
CDN_EVAL_HD void write_row(double *dst, const float *b, int cls, int coco) {
  if (coco) {
    const float w = b[2] - b[0], h = b[3] - b[1];       // formed in float32, as the reference's in-place subtraction
    dst[0] = cut2(b[0]);
    dst[1] = cut2(b[1]);
    dst[2] = cut2(w);
    dst[3] = cut2(h);
    dst[4] = cut2(b[4]);
  } else {
    for (int k = 0; k < 5; ++k) dst[k] = (double)b[k];
  }
  dst[5] = (double)cls;
}

// rows [0, n) of image `b` of a merge block behind `base` rows already in the slot; lane tid of nth.  pre[c] = rows of
// the classes before c (pre[classes] = all).  Rows that would land beyond cap are not stored: the caller raises the flag.
CDN_EVAL_HD void append_image(const float *boxes, const int *pre, int b, int classes, int R, double *det_img, int base, int cap,
                              int coco, int tid, int nth) {
  for (int c = 0; c < classes; ++c) {
    const int n = pre[c + 1] - pre[c];
    for (int r = tid; r < n; r += nth) {
      const int idx = base + pre[c] + r;
      if (idx < cap) write_row(det_img + (int64_t)idx * kCols, boxes + (((int64_t)b * classes + c) * R + r) * 5, c, coco);
    }
  }
}
CDN_EVAL_HD int clamp_rows(int r, int R) { return r < 0 ? 0 : (r > R ? R : r); }

// 64-bit key of one table row: (category, inverted orderable score); an ascending stable sort over the table's own order
// gives, per category, descending score with ties in (image, row) order.  VOC scores are exact float32; COCO scores are
// k / 100 and k is the key.  Rows behind an image's count sort behind every category.
CDN_EVAL_HD int64_t sort_key(const double *row, bool valid, int classes, int coco, int *bad) {
  CDN_EVAL_NOFMA
  if (!valid) return (int64_t)classes << 32;
  uint32_t ord;
  if (coco) {
    double k = rint(row[4] * 100.0);
    if (!(k >= -2147483648.0 && k <= 2147483647.0)) {
      *bad = 1;
      k = 0.0;
    }
    ord = (uint32_t)((int64_t)k + 2147483648LL);
  } else {
    float f = (float)row[4];
    if (f != f) *bad = 1;
    if (f == 0.0f) f = 0.0f;                // -0 and +0 are one score
    uint32_t u;
    memcpy(&u, &f, 4);
    ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((int64_t)(int)row[5] << 32) | (int64_t)(0xFFFFFFFFu - ord);
}

// "row j comes before row i" as a TOTAL order on any scores: descending, a NaN behind every number, ties (and NaNs among
// themselves) by index.  Ranks under a total order are a permutation of 0 .. D-1, so every slot of a ranked list is written
// whatever the network produced; a NaN is reported by the sort key's flag, after the match, and the final call raises.
CDN_EVAL_HD bool score_before(double sj, int j, double s, int i) {
  const bool jn = sj != sj, in = s != s;
  if (jn != in) return in;
  if (!jn && sj != s) return sj > s;
  return j < i;
}
// rank of row i among the rows of its own class in one image: descending score, stable
CDN_EVAL_HD int rank_of(const double *tab, int n, int i) {
  const double cls = tab[(int64_t)i * kCols + 5], s = tab[(int64_t)i * kCols + 4];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    if (j == i || tab[(int64_t)j * kCols + 5] != cls) continue;
    r += score_before(tab[(int64_t)j * kCols + 4], j, s, i) ? 1 : 0;
  }
  return r;
}
// the ranked rows of one (image, class) on one lane: order [min(D, keep)] <- rows by rank, every row's rank to rank_out
// when given.  Returns the number kept.  (The kernels' wave_rank is this loop strided over the lanes.)
CDN_EVAL_HD int rank_rows(const double *tab, int n, int cls, int keep, int *order, int *rank_out) {
  int d = 0;
  for (int i = 0; i < n; ++i) {
    if ((int)tab[(int64_t)i * kCols + 5] != cls) continue;
    const int r = rank_of(tab, n, i);
    if (rank_out) rank_out[i] = r;
    if (r < keep) order[r] = i;
    ++d;
  }
  return d < keep ? d : keep;
}

template <typename T>
CDN_EVAL_HD int64_t lower_bound(const T *a, int64_t lo, int64_t hi, T v) {      // first index in [lo, hi) with a[i] >= v
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- VOC (voc_eval.py:95-207) ------------------------------------------------------------------------------------------
CDN_EVAL_HD double voc_overlap(const double *d, const double *g) {
  CDN_EVAL_NOFMA
  const double ixmin = g[0] > d[0] ? g[0] : d[0], iymin = g[1] > d[1] ? g[1] : d[1];
  const double ixmax = g[2] < d[2] ? g[2] : d[2], iymax = g[3] < d[3] ? g[3] : d[3];
  double iw = (ixmax - ixmin) + 1.0, ih = (iymax - iymin) + 1.0;
  iw = iw > 0.0 ? iw : 0.0;
  ih = ih > 0.0 ? ih : 0.0;
  const double inter = iw * ih;
  const double da = ((d[2] - d[0]) + 1.0) * ((d[3] - d[1]) + 1.0), ga = ((g[2] - g[0]) + 1.0) * ((g[3] - g[1]) + 1.0);
  const double uni = (da + ga) - inter;
  return inter / uni;
}
// numpy's argmax as a total order: the first maximum, a NaN above every number
CDN_EVAL_HD bool voc_better(double ov, int idx, double bov, int bidx) {
  if (idx < 0) return false;
  if (bidx < 0) return true;
  const bool an = ov != ov, bn = bov != bov;
  if (an != bn) return an;
  if (!an && ov != bov) return ov > bov;
  return idx < bidx;
}
// lane 0's step behind the argmax: (tp, fp) of the detection; marks the box seen
CDN_EVAL_HD void voc_classify(double ovmax, int jmax, double ovthresh, const int *gt_flag, unsigned char *seen, unsigned char *tp,
                              unsigned char *fp) {
  *tp = 0;
  *fp = 0;
  if (jmax >= 0 && ovmax > ovthresh) {
    if (!(gt_flag[jmax] & 1)) {
      if (!seen[jmax]) {
        *tp = 1;
        seen[jmax] = 1;
      } else {
        *fp = 1;
      }
    }
  } else {
    *fp = 1;
  }
}
CDN_EVAL_HD double voc_rec(int64_t tp, int64_t npos) { return (double)tp / (double)(npos > 1 ? npos : 1); }
CDN_EVAL_HD double voc_prec(int64_t tp, int64_t fp) {
  const double s = (double)(tp + fp);
  return (double)tp / (s > DBL_EPSILON ? s : DBL_EPSILON);
}
CDN_EVAL_HD double voc_term(double rec, double prev, double env) {
  CDN_EVAL_NOFMA
  const double w = rec - prev;
  return w * env;
}
// numpy's float64 add.reduce over a contiguous array (pairwise, blocks of 128, eight running sums), without recursion:
// the split points are those of the recursive form, walked with an explicit stack
CDN_EVAL_HD double np_block_sum(const double *a, int64_t n) {
  if (n < 8) {
    double res = 0.0;
    for (int64_t i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int64_t i;
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}
CDN_EVAL_HD double np_pairwise_sum(const double *a, int64_t n) {
  // post-order walk: frames hold (offset, length, state, left value)
  int64_t off[48], len[48];
  double left[48];
  int state[48], sp = 0;
  off[0] = 0; len[0] = n; state[0] = 0; left[0] = 0.0;
  double ret = 0.0;
  while (sp >= 0) {
    if (len[sp] <= 128) {
      ret = np_block_sum(a + off[sp], len[sp]);
      --sp;
      continue;
    }
    int64_t n2 = len[sp] / 2;
    n2 -= n2 % 8;
    if (state[sp] == 0) {
      state[sp] = 1;
      off[sp + 1] = off[sp]; len[sp + 1] = n2; state[sp + 1] = 0;
      ++sp;
    } else if (state[sp] == 1) {
      left[sp] = ret;
      state[sp] = 2;
      off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; state[sp + 1] = 0;
      ++sp;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

// ---- COCO (COCOeval.evaluateImg / accumulate, iouType = "bbox") -----------------------------------------------------------
CDN_EVAL_HD double bb_iou(const double *d, const double *g, bool crowd) {
  CDN_EVAL_NOFMA
  const double dr = d[0] + d[2], gr = g[0] + g[2];
  const double w = (dr < gr ? dr : gr) - (d[0] > g[0] ? d[0] : g[0]);
  if (w <= 0.0) return 0.0;
  const double db = d[1] + d[3], gb = g[1] + g[3];
  const double h = (db < gb ? db : gb) - (d[1] > g[1] ? d[1] : g[1]);
  if (h <= 0.0) return 0.0;
  const double i = w * h, da = d[2] * d[3], ga = g[2] * g[3];
  const double u = crowd ? da : (da + ga) - i;
  return i / u;
}
struct CocoImg {
  const double *tab;      // the image's table rows
  const int *order;       // [D] ranked rows
  int D;
  const double *gt;       // [G][4] x y w h of this (image, category)
  const double *gt_area;  // [G]
  const int *gt_flag;     // [G] bit 0: iscrowd
  int G;
  const double *iou;      // [D][G] or nullptr: formed on the fly (the same function, the same bits)
};
CDN_EVAL_HD double coco_iou_at(const CocoImg &c, int d, int g) {
  return c.iou ? c.iou[(int64_t)d * c.G + g] : bb_iou(c.tab + (int64_t)c.order[d] * kCols, c.gt + (int64_t)g * 4, c.gt_flag[g] & 1);
}
CDN_EVAL_HD bool gt_ignored(const CocoImg &c, int g, double lo, double hi) {
  return (c.gt_flag[g] & 1) || c.gt_area[g] < lo || c.gt_area[g] > hi;
}
// one (IoU threshold, area range) matcher over the ranked detections of one (image, category); gtm [G] is its own.
// dtm / dtig are indexed by the image's table row.  Returns the number of ground truths it does not ignore.
CDN_EVAL_HD int coco_match_lane(const CocoImg &c, double thr, double lo, double hi, unsigned char *gtm, unsigned char *dtm,
                                unsigned char *dtig) {
  CDN_EVAL_NOFMA
  int nonign = 0;
  for (int g = 0; g < c.G; ++g) {
    gtm[g] = 0;
    nonign += gt_ignored(c, g, lo, hi) ? 0 : 1;
  }
  const double cap1 = 1.0 - 1e-10;
  for (int d = 0; d < c.D; ++d) {
    double best = thr < cap1 ? thr : cap1;
    int m = -1;
    // non-ignored ground truths first, in their own order, then the ignored ones -- which are not visited once a
    // non-ignored one is held
    for (int pass = 0; pass < 2 && m < 0; ++pass) {
      for (int g = 0; g < c.G; ++g) {
        if ((gt_ignored(c, g, lo, hi) ? 1 : 0) != pass) continue;
        if (gtm[g] && !(c.gt_flag[g] & 1)) continue;
        const double o = coco_iou_at(c, d, g);
        if (o < best) continue;
        best = o;
        m = g;
      }
    }
    const double *row = c.tab + (int64_t)c.order[d] * kCols;
    bool ig;
    if (m >= 0) {
      ig = gt_ignored(c, m, lo, hi);
      gtm[m] = 1;
    } else {
      const double area = row[2] * row[3];
      ig = area < lo || area > hi;
    }
    dtm[c.order[d]] = m >= 0 ? 1 : 0;
    dtig[c.order[d]] = ig ? 1 : 0;
  }
  return nonign;
}
CDN_EVAL_HD double coco_rc(int64_t tp, int64_t npig) { return (double)tp / (double)npig; }
CDN_EVAL_HD double coco_pr(int64_t tp, int64_t fp) {
  CDN_EVAL_NOFMA
  const double s = (double)(fp + tp) + 2.220446049250313e-16;
  return (double)tp / s;
}
// how many recall thresholds lie at or below rc: the detection's precision counts for thresholds [0, that)
CDN_EVAL_HD int rec_bucket(const double *rec_thrs, double rc) {
  int lo = 0, hi = kRec;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (rec_thrs[mid] <= rc) lo = mid + 1; else hi = mid;
  }
  return lo;
}
CDN_EVAL_HD int64_t precision_index(int t, int r, int k, int a, int m, int K) {
  return ((((int64_t)t * kRec + r) * K + k) * kAreas + a) * kMaxDetsN + m;
}
CDN_EVAL_HD int64_t recall_index(int t, int k, int a, int m, int K) {
  return (((int64_t)t * K + k) * kAreas + a) * kMaxDetsN + m;
}

}  // namespace cdn_eval
