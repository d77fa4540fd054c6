// codenet_eval.hip -- detection scoring on the device: VOC07 AP per class and COCO's bbox precision / recall arrays from a
// float64 detection table that the merge block of cdn_ctdet_merge_scales is appended to.  DESIGN.md section 7.4e is the
// contract; the arithmetic is cdn_eval.h, plain C++ that the kernels here and the cdn_eval_*_host entries both run.
//
// ---- the kernels -----------------------------------------------------------------------------------------------------
// eval_append_kernel        one workgroup per image of the block: class prefix on thread 0, rows by all threads; rows
//                           beyond cap raise bit 0 of the flag word and are not stored.
// eval_keys_kernel          one thread per table row: the 64-bit sort key (category, inverted orderable score).
// eval_match_voc_kernel     one wave per (image, class): stable rank in LDS, then per detection in rank order the lanes
//                           form the overlaps, a shuffle tree takes numpy's argmax (a total order: any tree gives the
//                           same answer) and lane 0 books TP / FP / seen.
// eval_match_coco_kernel    one wave per (image, category): rank, the D x G IoU matrix in LDS when it fits (formed on
//                           the fly by the same function otherwise), then lanes 0..39 are the 10 x 4 sequential matchers.
// eval_accumulate_voc_kernel   one workgroup per class over its segment of the sorted table: integer scans of TP / FP,
//                           rec / prec per element, a max-scan from the right for the envelope, the compacted area terms;
//                           thread 0 reads the 11 points and sums the terms in numpy's pairwise order.
// eval_accumulate_coco_kernel  one workgroup per (category, area range, maxDets, IoU threshold): integer scans, and per
//                           detection an LDS integer max of its precision's bit pattern into the bucket of the recall
//                           thresholds it reaches; a max from the right over the 101 buckets is accumulate's q.
// Everything that crosses lanes is an integer count or a maximum: no order of execution can change a bit.
#include "cdn_common.h"
#include "cdn_eval.h"

namespace {

namespace E = cdn_eval;
constexpr int kThreads = 256;

struct Table {
  const double *det;
  const int *count;
  int n_images, cap, classes;
};
struct Gt {
  const double *box, *area;
  const int *flag, *off;
};

// ---- append ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) eval_append_kernel(const float *boxes, const int *rows_out, int classes, int R,
                                                               int slot0, double *det, int *count, int cap, int coco,
                                                               int *flag) {
  __shared__ int s_pre[E::kMaxClasses + 1];
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int c = 0; c < classes; ++c) {
      s_pre[c] = acc;
      acc += E::clamp_rows(rows_out[b * classes + c], R);
    }
    s_pre[classes] = acc;
  }
  __syncthreads();
  const int base = count[slot0 + b];
  E::append_image(boxes, s_pre, b, classes, R, det + (int64_t)(slot0 + b) * cap * E::kCols, base, cap, coco, threadIdx.x,
                  kThreads);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = base + s_pre[classes];
    if (total > cap) atomicOr(flag, (int)E::kFlagOverflow);
    count[slot0 + b] = total > cap ? cap : total;
  }
}

void append_host(const float *boxes, const int *rows_out, int B, int classes, int R, int slot0, double *det, int *count,
                 int cap, int coco, int *flag) {
  int pre[E::kMaxClasses + 1];
  for (int b = 0; b < B; ++b) {
    int acc = 0;
    for (int c = 0; c < classes; ++c) {
      pre[c] = acc;
      acc += E::clamp_rows(rows_out[b * classes + c], R);
    }
    pre[classes] = acc;
    const int base = count[slot0 + b];
    E::append_image(boxes, pre, b, classes, R, det + (int64_t)(slot0 + b) * cap * E::kCols, base, cap, coco, 0, 1);
    const int total = base + acc;
    if (total > cap) *flag |= E::kFlagOverflow;
    count[slot0 + b] = total > cap ? cap : total;
  }
}

// ---- keys --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) eval_keys_kernel(Table t, int coco, int64_t *keys, int *flag) {
  const int64_t n = (int64_t)t.n_images * t.cap;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int img = (int)(i / t.cap), row = (int)(i % t.cap);
    int bad = 0;
    keys[i] = E::sort_key(t.det + i * E::kCols, row < t.count[img], t.classes, coco, &bad);
    if (bad) atomicOr(flag, (int)E::kFlagScore);
  }
}

void keys_host(Table t, int coco, int64_t *keys, int *flag) {
  const int64_t n = (int64_t)t.n_images * t.cap;
  for (int64_t i = 0; i < n; ++i) {
    int bad = 0;
    keys[i] = E::sort_key(t.det + i * E::kCols, (int)(i % t.cap) < t.count[i / t.cap], t.classes, coco, &bad);
    if (bad) *flag |= E::kFlagScore;
  }
}

// ---- the ranked rows of one (image, class), shared by the two match kernels -----------------------------------------------
// s_order [min(cap, keep)] <- rows by rank; every row's rank goes to rank_out when given.  Returns the number kept.
__device__ __forceinline__ int wave_rank(const double *tab, int n, int cls, int keep, int *s_order, int *s_count, int *rank_out) {
  const int lane = threadIdx.x;
  if (lane == 0) *s_count = 0;
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    if ((int)tab[(int64_t)i * E::kCols + 5] != cls) continue;
    const int r = E::rank_of(tab, n, i);
    if (rank_out) rank_out[i] = r;
    if (r < keep) s_order[r] = i;
    atomicAdd(s_count, 1);
  }
  __syncthreads();
  const int d = *s_count;
  return d < keep ? d : keep;
}

// ---- VOC match -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) eval_match_voc_kernel(Table t, Gt gt, double ovthresh, unsigned char *seen, unsigned char *tp,
                                                            unsigned char *fp) {
  __shared__ int s_order[E::kMaxCap];
  __shared__ int s_count;
  const int ic = blockIdx.x, img = ic / t.classes, cls = ic % t.classes, lane = threadIdx.x;
  const int n = min(t.count[img], t.cap);
  const double *tab = t.det + (int64_t)img * t.cap * E::kCols;
  const int D = wave_rank(tab, n, cls, t.cap, s_order, &s_count, nullptr);
  const int g0 = gt.off[ic], G = gt.off[ic + 1] - g0;
  for (int g = lane; g < G; g += 64) seen[g0 + g] = 0;
  __syncthreads();
  for (int d = 0; d < D; ++d) {
    const int row = s_order[d];
    double best = 0.0;
    int bidx = -1;
    for (int g = lane; g < G; g += 64) {
      const double ov = E::voc_overlap(tab + (int64_t)row * E::kCols, gt.box + (int64_t)(g0 + g) * 4);
      if (E::voc_better(ov, g, best, bidx)) {
        best = ov;
        bidx = g;
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const double o = __shfl_xor(best, m, 64);
      const int oi = __shfl_xor(bidx, m, 64);
      if (E::voc_better(o, oi, best, bidx)) {
        best = o;
        bidx = oi;
      }
    }
    if (lane == 0)
      E::voc_classify(best, bidx, ovthresh, gt.flag + g0, seen + g0, tp + (int64_t)img * t.cap + row,
                      fp + (int64_t)img * t.cap + row);
  }
}

void match_voc_host(Table t, Gt gt, double ovthresh, unsigned char *seen, unsigned char *tp, unsigned char *fp, int *order) {
  for (int ic = 0; ic < t.n_images * t.classes; ++ic) {
    const int img = ic / t.classes, cls = ic % t.classes;
    const int n = t.count[img] < t.cap ? t.count[img] : t.cap;
    const double *tab = t.det + (int64_t)img * t.cap * E::kCols;
    const int D = E::rank_rows(tab, n, cls, t.cap, order, nullptr);
    const int g0 = gt.off[ic], G = gt.off[ic + 1] - g0;
    for (int g = 0; g < G; ++g) seen[g0 + g] = 0;
    for (int d = 0; d < D; ++d) {
      const int row = order[d];
      double best = 0.0;
      int bidx = -1;
      for (int g = 0; g < G; ++g) {
        const double ov = E::voc_overlap(tab + (int64_t)row * E::kCols, gt.box + (int64_t)(g0 + g) * 4);
        if (E::voc_better(ov, g, best, bidx)) {
          best = ov;
          bidx = g;
        }
      }
      E::voc_classify(best, bidx, ovthresh, gt.flag + g0, seen + g0, tp + (int64_t)img * t.cap + row,
                      fp + (int64_t)img * t.cap + row);
    }
  }
}

// ---- COCO match ----------------------------------------------------------------------------------------------------------
struct CocoMatch {
  const double *iou_thrs, *area_rng;      // [10], [4][2]
  unsigned char *gtm, *dtm, *dtig;        // [40][total_gt], [40][n_images * cap] twice
  int *rank, *gt_nonign;                  // [n_images * cap], [n_images * classes][4]
  int64_t total_gt;
};

__global__ void __launch_bounds__(64) eval_match_coco_kernel(Table t, Gt gt, CocoMatch m) {
  __shared__ int s_order[E::kMaxDet];
  __shared__ int s_count;
  __shared__ double s_iou[E::kLdsIou];
  const int ic = blockIdx.x, img = ic / t.classes, cls = ic % t.classes, lane = threadIdx.x;
  const int n = min(t.count[img], t.cap);
  const int64_t ntab = (int64_t)t.n_images * t.cap;
  E::CocoImg c;
  c.tab = t.det + (int64_t)img * t.cap * E::kCols;
  c.D = wave_rank(c.tab, n, cls, E::kMaxDet, s_order, &s_count, m.rank + (int64_t)img * t.cap);
  c.order = s_order;
  const int g0 = gt.off[ic];
  c.G = gt.off[ic + 1] - g0;
  c.gt = gt.box + (int64_t)g0 * 4;
  c.gt_area = gt.area + g0;
  c.gt_flag = gt.flag + g0;
  c.iou = nullptr;
  if ((int64_t)c.D * c.G <= E::kLdsIou) {
    for (int k = lane; k < c.D * c.G; k += 64) s_iou[k] = E::coco_iou_at(c, k / c.G, k % c.G);
    __syncthreads();
    c.iou = s_iou;
  }
  if (lane < E::kLanes) {
    const int ti = lane / E::kAreas, a = lane % E::kAreas;
    const int nonign = E::coco_match_lane(c, m.iou_thrs[ti], m.area_rng[2 * a], m.area_rng[2 * a + 1],
                                          m.gtm + (int64_t)lane * m.total_gt + g0, m.dtm + lane * ntab + (int64_t)img * t.cap,
                                          m.dtig + lane * ntab + (int64_t)img * t.cap);
    if (ti == 0) m.gt_nonign[(int64_t)ic * E::kAreas + a] = nonign;
  }
}

void match_coco_host(Table t, Gt gt, CocoMatch m) {
  int order[E::kMaxDet];
  const int64_t ntab = (int64_t)t.n_images * t.cap;
  for (int ic = 0; ic < t.n_images * t.classes; ++ic) {
    const int img = ic / t.classes, cls = ic % t.classes;
    const int n = t.count[img] < t.cap ? t.count[img] : t.cap;
    E::CocoImg c;
    c.tab = t.det + (int64_t)img * t.cap * E::kCols;
    c.D = E::rank_rows(c.tab, n, cls, E::kMaxDet, order, m.rank + (int64_t)img * t.cap);
    c.order = order;
    const int g0 = gt.off[ic];
    c.G = gt.off[ic + 1] - g0;
    c.gt = gt.box + (int64_t)g0 * 4;
    c.gt_area = gt.area + g0;
    c.gt_flag = gt.flag + g0;
    c.iou = nullptr;
    for (int lane = 0; lane < E::kLanes; ++lane) {
      const int ti = lane / E::kAreas, a = lane % E::kAreas;
      const int nonign = E::coco_match_lane(c, m.iou_thrs[ti], m.area_rng[2 * a], m.area_rng[2 * a + 1],
                                            m.gtm + (int64_t)lane * m.total_gt + g0, m.dtm + lane * ntab + (int64_t)img * t.cap,
                                            m.dtig + lane * ntab + (int64_t)img * t.cap);
      if (ti == 0) m.gt_nonign[(int64_t)ic * E::kAreas + a] = nonign;
    }
  }
}

// ---- workgroup scans -------------------------------------------------------------------------------------------------------
// inclusive sums of (a, b) over the 256 threads in thread order; tot: the workgroup's totals.  s: 8 ints of LDS.
__device__ __forceinline__ void block_scan2(int &a, int &b, int &tot_a, int &tot_b, int *s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ua = __shfl_up(a, d, 64), ub = __shfl_up(b, d, 64);
    if (lane >= d) {
      a += ua;
      b += ub;
    }
  }
  __syncthreads();
  if (lane == 63) {
    s[2 * wave] = a;
    s[2 * wave + 1] = b;
  }
  __syncthreads();
  tot_a = 0;
  tot_b = 0;
  for (int w = 0; w < kThreads / 64; ++w) {
    if (w < wave) {
      a += s[2 * w];
      b += s[2 * w + 1];
    }
    tot_a += s[2 * w];
    tot_b += s[2 * w + 1];
  }
}
// inclusive maximum over the 256 threads in thread order (v >= 0); tot: the workgroup's maximum.  s: 4 doubles of LDS.
__device__ __forceinline__ void block_scan_max(double &v, double &tot, double *s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double u = __shfl_up(v, d, 64);
    if (lane >= d) v = u > v ? u : v;
  }
  __syncthreads();
  if (lane == 63) s[wave] = v;
  __syncthreads();
  tot = 0.0;
  for (int w = 0; w < kThreads / 64; ++w) {
    if (w < wave) v = s[w] > v ? s[w] : v;
    tot = s[w] > tot ? s[w] : tot;
  }
}
__device__ __forceinline__ int block_sum(int v, int *s) {
  __syncthreads();
  if (threadIdx.x == 0) *s = 0;
  __syncthreads();
  atomicAdd(s, v);
  __syncthreads();
  return *s;
}

// ---- VOC accumulate ------------------------------------------------------------------------------------------------------
struct VocAcc {
  const int64_t *keys, *perm;      // the sorted keys and the table rows behind them
  const unsigned char *tp, *fp;
  const double *thr;               // [n_thr] the recall points, from the host
  int n_thr;
  const int *flag;
  double *rec, *prec, *env, *terms;   // [n], [n], [n], [n + classes]
  double *out;                     // ap_07 [classes], ap_area [classes], npos [classes], seg_off [classes + 1], flag
};
__host__ __device__ inline void voc_finish(const VocAcc &a, int c, int classes, int64_t s0, int64_t s1, int64_t npos, int64_t nterm) {
  // thread 0 / the host: the closing term of mrec = [.., 1], the two APs, the bookkeeping
  double *terms = a.terms + s0 + c;
  const double last = s1 > s0 ? a.rec[s1 - 1] : 0.0;
  if (1.0 != last) terms[nterm++] = E::voc_term(1.0, last, 0.0);
  double ap = 0.0;
  for (int k = 0; k < a.n_thr; ++k) {
    const int64_t i = E::lower_bound(a.rec, s0, s1, a.thr[k]);
    const double p = i < s1 ? a.env[i] : 0.0;
    ap = ap + p / (double)a.n_thr;
  }
  a.out[c] = ap;
  a.out[classes + c] = E::np_pairwise_sum(terms, nterm);
  a.out[2 * classes + c] = (double)npos;
  a.out[3 * classes + c] = (double)s0;
  if (c == classes - 1) {
    a.out[3 * classes + classes] = (double)s1;
    a.out[4 * classes + 1] = (double)*a.flag;
  }
}

__global__ void __launch_bounds__(kThreads) eval_accumulate_voc_kernel(Table t, Gt gt, VocAcc a) {
  __shared__ int s_i[8], s_sum;
  __shared__ double s_d[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t n = (int64_t)t.n_images * t.cap;
  const int64_t s0 = E::lower_bound(a.keys, (int64_t)0, n, (int64_t)c << 32);
  const int64_t s1 = E::lower_bound(a.keys, s0, n, (int64_t)(c + 1) << 32);
  int mine = 0;
  for (int img = tid; img < t.n_images; img += kThreads)
    for (int g = gt.off[img * t.classes + c]; g < gt.off[img * t.classes + c + 1]; ++g) mine += (gt.flag[g] & 1) ? 0 : 1;
  const int64_t npos = block_sum(mine, &s_sum);
  // left to right: cumulative TP / FP, rec, prec
  int64_t ctp = 0, cfp = 0;
  for (int64_t base = s0; base < s1; base += kThreads) {
    const int64_t i = base + tid;
    int x = 0, y = 0, tx, ty;
    if (i < s1) {
      x = a.tp[a.perm[i]];
      y = a.fp[a.perm[i]];
    }
    block_scan2(x, y, tx, ty, s_i);
    if (i < s1) {
      a.rec[i] = E::voc_rec(ctp + x, npos);
      a.prec[i] = E::voc_prec(ctp + x, cfp + y);
    }
    ctp += tx;
    cfp += ty;
  }
  __syncthreads();
  // right to left: the monotone envelope
  double carry = 0.0;
  for (int64_t base = s1; base > s0; base -= kThreads) {
    const int64_t i = base - 1 - tid;
    double v = i >= s0 ? a.prec[i] : 0.0, tot;
    block_scan_max(v, tot, s_d);
    if (i >= s0) a.env[i] = carry > v ? carry : v;
    carry = tot > carry ? tot : carry;
  }
  __syncthreads();
  // left to right: the terms of the area sum, compacted in order
  int64_t nterm = 0;
  for (int64_t base = s0; base < s1; base += kThreads) {
    const int64_t i = base + tid;
    int x = 0, y = 0, tx, ty;
    double prev = 0.0;
    if (i < s1) {
      prev = i > s0 ? a.rec[i - 1] : 0.0;
      x = a.rec[i] != prev ? 1 : 0;
    }
    const int has = x;
    block_scan2(x, y, tx, ty, s_i);
    if (has) a.terms[s0 + c + nterm + x - 1] = E::voc_term(a.rec[i], prev, a.env[i]);
    nterm += tx;
  }
  __syncthreads();
  if (tid == 0) voc_finish(a, c, t.classes, s0, s1, npos, nterm);
}

void accumulate_voc_host(Table t, Gt gt, VocAcc a) {
  const int64_t n = (int64_t)t.n_images * t.cap;
  for (int c = 0; c < t.classes; ++c) {
    const int64_t s0 = E::lower_bound(a.keys, (int64_t)0, n, (int64_t)c << 32);
    const int64_t s1 = E::lower_bound(a.keys, s0, n, (int64_t)(c + 1) << 32);
    int64_t npos = 0;
    for (int img = 0; img < t.n_images; ++img)
      for (int g = gt.off[img * t.classes + c]; g < gt.off[img * t.classes + c + 1]; ++g) npos += (gt.flag[g] & 1) ? 0 : 1;
    int64_t ctp = 0, cfp = 0;
    for (int64_t i = s0; i < s1; ++i) {
      ctp += a.tp[a.perm[i]];
      cfp += a.fp[a.perm[i]];
      a.rec[i] = E::voc_rec(ctp, npos);
      a.prec[i] = E::voc_prec(ctp, cfp);
    }
    double carry = 0.0;
    for (int64_t i = s1 - 1; i >= s0; --i) {
      carry = a.prec[i] > carry ? a.prec[i] : carry;
      a.env[i] = carry;
    }
    int64_t nterm = 0;
    for (int64_t i = s0; i < s1; ++i) {
      const double prev = i > s0 ? a.rec[i - 1] : 0.0;
      if (a.rec[i] != prev) a.terms[s0 + c + nterm++] = E::voc_term(a.rec[i], prev, a.env[i]);
    }
    voc_finish(a, c, t.classes, s0, s1, npos, nterm);
  }
}

// ---- COCO accumulate -----------------------------------------------------------------------------------------------------
struct CocoAcc {
  const int64_t *keys, *perm;
  const unsigned char *dtm, *dtig;
  const int *rank, *gt_nonign;
  const double *rec_thrs;          // [101]
  const int *flag;
  double *precision, *recall;      // [10][101][K][4][3], [10][K][4][3]
  double *flag_out;
};
__host__ __device__ inline void coco_finish(const CocoAcc &a, int ti, int k, int ar, int m, int K, int64_t npig, int64_t nd,
                                            int64_t tp_total, const unsigned long long *best) {
  if (npig == 0) {
    for (int r = 0; r < E::kRec; ++r) a.precision[E::precision_index(ti, r, k, ar, m, K)] = -1.0;
    a.recall[E::recall_index(ti, k, ar, m, K)] = -1.0;
  } else {
    unsigned long long run = 0;      // precisions are >= 0: their bit patterns order as they do
    for (int r = E::kRec - 1; r >= 0; --r) {
      run = best[r] > run ? best[r] : run;
      double q;
      memcpy(&q, &run, 8);
      a.precision[E::precision_index(ti, r, k, ar, m, K)] = q;
    }
    a.recall[E::recall_index(ti, k, ar, m, K)] = nd ? E::coco_rc(tp_total, npig) : 0.0;
  }
  if (ti == 0 && k == 0 && ar == 0 && m == 0) *a.flag_out = (double)*a.flag;
}

__global__ void __launch_bounds__(kThreads) eval_accumulate_coco_kernel(Table t, CocoAcc a) {
  __shared__ int s_i[8], s_sum;
  __shared__ unsigned long long s_best[E::kRec];
  const int k = blockIdx.x, ar = blockIdx.y / E::kMaxDetsN, m = blockIdx.y % E::kMaxDetsN, ti = blockIdx.z, tid = threadIdx.x;
  const int lane = ti * E::kAreas + ar, keep = E::max_dets(m);
  const int64_t n = (int64_t)t.n_images * t.cap;
  const int64_t s0 = E::lower_bound(a.keys, (int64_t)0, n, (int64_t)k << 32);
  const int64_t s1 = E::lower_bound(a.keys, s0, n, (int64_t)(k + 1) << 32);
  int mine = 0;
  for (int img = tid; img < t.n_images; img += kThreads) mine += a.gt_nonign[((int64_t)img * t.classes + k) * E::kAreas + ar];
  const int64_t npig = block_sum(mine, &s_sum);
  for (int r = tid; r < E::kRec; r += kThreads) s_best[r] = 0;
  __syncthreads();
  int64_t ctp = 0, cfp = 0, nd = 0;
  if (npig > 0) {
    for (int64_t base = s0; base < s1; base += kThreads) {
      const int64_t i = base + tid;
      int x = 0, y = 0, tx, ty, inc = 0;
      if (i < s1) {
        const int64_t row = a.perm[i];
        inc = a.rank[row] < keep ? 1 : 0;
        const int mt = a.dtm[lane * n + row], ig = a.dtig[lane * n + row];
        x = (inc && mt && !ig) ? 1 : 0;
        y = (inc && !mt && !ig) ? 1 : 0;
      }
      block_scan2(x, y, tx, ty, s_i);
      if (inc) {
        const double pr = E::coco_pr(ctp + x, cfp + y);
        const int b = E::rec_bucket(a.rec_thrs, E::coco_rc(ctp + x, npig));
        unsigned long long bits;
        memcpy(&bits, &pr, 8);
        if (b > 0) atomicMax(&s_best[b - 1], bits);
      }
      ctp += tx;
      cfp += ty;
      nd += block_sum(inc, &s_sum);
    }
  }
  __syncthreads();
  if (tid == 0) coco_finish(a, ti, k, ar, m, t.classes, npig, nd, ctp, s_best);
}

void accumulate_coco_host(Table t, CocoAcc a) {
  const int64_t n = (int64_t)t.n_images * t.cap;
  unsigned long long best[E::kRec];
  for (int k = 0; k < t.classes; ++k) {
    const int64_t s0 = E::lower_bound(a.keys, (int64_t)0, n, (int64_t)k << 32);
    const int64_t s1 = E::lower_bound(a.keys, s0, n, (int64_t)(k + 1) << 32);
    for (int ar = 0; ar < E::kAreas; ++ar) {
      int64_t npig = 0;
      for (int img = 0; img < t.n_images; ++img) npig += a.gt_nonign[((int64_t)img * t.classes + k) * E::kAreas + ar];
      for (int m = 0; m < E::kMaxDetsN; ++m)
        for (int ti = 0; ti < E::kThr; ++ti) {
          const int lane = ti * E::kAreas + ar, keep = E::max_dets(m);
          for (int r = 0; r < E::kRec; ++r) best[r] = 0;
          int64_t ctp = 0, cfp = 0, nd = 0;
          for (int64_t i = s0; npig > 0 && i < s1; ++i) {
            const int64_t row = a.perm[i];
            if (a.rank[row] >= keep) continue;
            const int mt = a.dtm[lane * n + row], ig = a.dtig[lane * n + row];
            ctp += (mt && !ig) ? 1 : 0;
            cfp += (!mt && !ig) ? 1 : 0;
            ++nd;
            const double pr = E::coco_pr(ctp, cfp);
            const int b = E::rec_bucket(a.rec_thrs, E::coco_rc(ctp, npig));
            unsigned long long bits;
            memcpy(&bits, &pr, 8);
            if (b > 0 && bits > best[b - 1]) best[b - 1] = bits;
          }
          coco_finish(a, ti, k, ar, m, t.classes, npig, nd, ctp, best);
        }
    }
  }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------
int make_sizes(Table *t, int64_t n_images, int64_t cap, int64_t classes);
int make_table(Table *t, const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes) {
  CDN_REQUIRE(det && count, CDN_ERR_ARG, "null pointer");
  const int rc = make_sizes(t, n_images, cap, classes);
  t->det = det;
  t->count = count;
  return rc;
}
// the table's sizes alone (the accumulate entries read the sorted keys, not the rows)
int make_sizes(Table *t, int64_t n_images, int64_t cap, int64_t classes) {
  CDN_REQUIRE(n_images >= 1 && cap >= 1 && classes >= 1, CDN_ERR_ARG, "n_images, cap and classes must be positive");
  CDN_REQUIRE(cap <= E::kMaxCap, CDN_ERR_UNSUPPORTED, "cap %lld beyond %d rows per image", (long long)cap, E::kMaxCap);
  CDN_REQUIRE(classes <= E::kMaxClasses, CDN_ERR_UNSUPPORTED, "more than %d classes", E::kMaxClasses);
  CDN_REQUIRE(n_images * cap < (1LL << 31) / 64 && n_images * classes < (1LL << 31) / 4, CDN_ERR_UNSUPPORTED,
              "table of %lld x %lld rows too large", (long long)n_images, (long long)cap);
  *t = Table{nullptr, nullptr, (int)n_images, (int)cap, (int)classes};
  return CDN_OK;
}
int check_append(const float *boxes, const int32_t *rows_out, int64_t B, int64_t classes, int64_t R, int64_t image_slot,
                 double *det, int32_t *count, int64_t n_images, int64_t cap, int32_t *flag) {
  Table t;
  const int rc = make_table(&t, det, count, n_images, cap, classes);
  if (rc != CDN_OK) return rc;
  CDN_REQUIRE(boxes && rows_out && flag, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(B >= 1 && R >= 1 && R <= (1 << 20), CDN_ERR_ARG, "B and R must be positive");
  CDN_REQUIRE(image_slot >= 0 && image_slot + B <= n_images, CDN_ERR_ARG, "image slots %lld..%lld outside the table of %lld",
              (long long)image_slot, (long long)(image_slot + B - 1), (long long)n_images);
  CDN_REQUIRE(B * classes * R < (1LL << 31) / 5, CDN_ERR_UNSUPPORTED, "block too large");
  return CDN_OK;
}

}  // namespace

extern "C" int cdn_eval_append(const float *boxes, const int32_t *rows_out, int64_t B, int64_t classes, int64_t R,
                               int64_t image_slot, double *det, int32_t *count, int64_t n_images, int64_t cap, int coco,
                               int32_t *flag, void *stream) {
  const int rc = check_append(boxes, rows_out, B, classes, R, image_slot, det, count, n_images, cap, flag);
  if (rc != CDN_OK) return rc;
  eval_append_kernel<<<(unsigned)B, kThreads, 0, cdn::as_stream(stream)>>>(boxes, rows_out, (int)classes, (int)R, (int)image_slot,
                                                                         det, count, (int)cap, coco ? 1 : 0, flag);
  return cdn::check_launch("eval append");
}
extern "C" int cdn_eval_append_host(const float *boxes, const int32_t *rows_out, int64_t B, int64_t classes, int64_t R,
                                    int64_t image_slot, double *det, int32_t *count, int64_t n_images, int64_t cap, int coco,
                                    int32_t *flag) {
  const int rc = check_append(boxes, rows_out, B, classes, R, image_slot, det, count, n_images, cap, flag);
  if (rc != CDN_OK) return rc;
  append_host(boxes, rows_out, (int)B, (int)classes, (int)R, (int)image_slot, det, count, (int)cap, coco ? 1 : 0, flag);
  return CDN_OK;
}

extern "C" int cdn_eval_sort_keys(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                  int coco, int64_t *keys, int32_t *flag, void *stream) {
  Table t;
  const int rc = make_table(&t, det, count, n_images, cap, classes);
  if (rc != CDN_OK) return rc;
  CDN_REQUIRE(keys && flag, CDN_ERR_ARG, "null pointer");
  const int64_t g = cdn::ceil_div(n_images * cap, kThreads);
  eval_keys_kernel<<<(unsigned)(g > 4096 ? 4096 : g), kThreads, 0, cdn::as_stream(stream)>>>(t, coco ? 1 : 0, keys, flag);
  return cdn::check_launch("eval keys");
}
extern "C" int cdn_eval_sort_keys_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                       int coco, int64_t *keys, int32_t *flag) {
  Table t;
  const int rc = make_table(&t, det, count, n_images, cap, classes);
  if (rc != CDN_OK) return rc;
  CDN_REQUIRE(keys && flag, CDN_ERR_ARG, "null pointer");
  keys_host(t, coco ? 1 : 0, keys, flag);
  return CDN_OK;
}

#define CDN_EVAL_VOC_MATCH_ARGS                                                                                              \
  Table t;                                                                                                                   \
  const int rc = make_table(&t, det, count, n_images, cap, classes);                                                         \
  if (rc != CDN_OK) return rc;                                                                                               \
  CDN_REQUIRE(gt_box && gt_flag && gt_off && seen && tp && fp, CDN_ERR_ARG, "null pointer");                                 \
  const Gt gt{gt_box, nullptr, gt_flag, gt_off};

extern "C" int cdn_eval_match_voc(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                  const double *gt_box, const int32_t *gt_flag, const int32_t *gt_off, double ovthresh,
                                  unsigned char *seen, unsigned char *tp, unsigned char *fp, void *stream) {
  CDN_EVAL_VOC_MATCH_ARGS
  eval_match_voc_kernel<<<(unsigned)(n_images * classes), 64, 0, cdn::as_stream(stream)>>>(t, gt, ovthresh, seen, tp, fp);
  return cdn::check_launch("eval match voc");
}
extern "C" int cdn_eval_match_voc_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                       const double *gt_box, const int32_t *gt_flag, const int32_t *gt_off, double ovthresh,
                                       unsigned char *seen, unsigned char *tp, unsigned char *fp) {
  CDN_EVAL_VOC_MATCH_ARGS
  int order[E::kMaxCap];
  match_voc_host(t, gt, ovthresh, seen, tp, fp, order);
  return CDN_OK;
}

#define CDN_EVAL_VOC_ACC_ARGS                                                                                                \
  Table t;                                                                                                                   \
  const int rc = make_sizes(&t, n_images, cap, classes);                                                                     \
  if (rc != CDN_OK) return rc;                                                                                               \
  CDN_REQUIRE(keys_sorted && perm && tp && fp && gt_flag && gt_off && thresholds && flag && rec && prec && env && terms && out, \
              CDN_ERR_ARG, "null pointer");                                                                                  \
  CDN_REQUIRE(n_thr >= 1 && n_thr <= 1024, CDN_ERR_ARG, "n_thr must be in [1, 1024]");                                       \
  const Gt gt{nullptr, nullptr, gt_flag, gt_off};                                                                            \
  const VocAcc a{keys_sorted, perm, tp, fp, thresholds, (int)n_thr, flag, rec, prec, env, terms, out};

extern "C" int cdn_eval_accumulate_voc(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                       int64_t classes, const unsigned char *tp, const unsigned char *fp, const int32_t *gt_flag,
                                       const int32_t *gt_off, const double *thresholds, int64_t n_thr, const int32_t *flag,
                                       double *rec, double *prec, double *env, double *terms, double *out, void *stream) {
  CDN_EVAL_VOC_ACC_ARGS
  eval_accumulate_voc_kernel<<<(unsigned)classes, kThreads, 0, cdn::as_stream(stream)>>>(t, gt, a);
  return cdn::check_launch("eval accumulate voc");
}
extern "C" int cdn_eval_accumulate_voc_host(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                            int64_t classes, const unsigned char *tp, const unsigned char *fp,
                                            const int32_t *gt_flag, const int32_t *gt_off, const double *thresholds,
                                            int64_t n_thr, const int32_t *flag, double *rec, double *prec, double *env,
                                            double *terms, double *out) {
  CDN_EVAL_VOC_ACC_ARGS
  accumulate_voc_host(t, gt, a);
  return CDN_OK;
}

#define CDN_EVAL_COCO_MATCH_ARGS                                                                                             \
  Table t;                                                                                                                   \
  const int rc = make_table(&t, det, count, n_images, cap, classes);                                                         \
  if (rc != CDN_OK) return rc;                                                                                               \
  CDN_REQUIRE(gt_box && gt_area && gt_flag && gt_off && iou_thrs && area_rng && gtm && dtm && dtig && rank && gt_nonign,     \
              CDN_ERR_ARG, "null pointer");                                                                                  \
  CDN_REQUIRE(total_gt >= 0 && total_gt < (1LL << 31) / E::kLanes, CDN_ERR_UNSUPPORTED, "too many ground truths");           \
  const Gt gt{gt_box, gt_area, gt_flag, gt_off};                                                                             \
  const CocoMatch m{iou_thrs, area_rng, gtm, dtm, dtig, rank, gt_nonign, total_gt};

extern "C" int cdn_eval_match_coco(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                   const double *gt_box, const double *gt_area, const int32_t *gt_flag, const int32_t *gt_off,
                                   int64_t total_gt, const double *iou_thrs, const double *area_rng, unsigned char *gtm,
                                   unsigned char *dtm, unsigned char *dtig, int32_t *rank, int32_t *gt_nonign, void *stream) {
  CDN_EVAL_COCO_MATCH_ARGS
  eval_match_coco_kernel<<<(unsigned)(n_images * classes), 64, 0, cdn::as_stream(stream)>>>(t, gt, m);
  return cdn::check_launch("eval match coco");
}
extern "C" int cdn_eval_match_coco_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                                        const double *gt_box, const double *gt_area, const int32_t *gt_flag,
                                        const int32_t *gt_off, int64_t total_gt, const double *iou_thrs, const double *area_rng,
                                        unsigned char *gtm, unsigned char *dtm, unsigned char *dtig, int32_t *rank,
                                        int32_t *gt_nonign) {
  CDN_EVAL_COCO_MATCH_ARGS
  match_coco_host(t, gt, m);
  return CDN_OK;
}

#define CDN_EVAL_COCO_ACC_ARGS                                                                                               \
  Table t;                                                                                                                   \
  const int rc = make_sizes(&t, n_images, cap, classes);                                                                     \
  if (rc != CDN_OK) return rc;                                                                                               \
  CDN_REQUIRE(keys_sorted && perm && dtm && dtig && rank && gt_nonign && rec_thrs && flag && precision && recall && flag_out, \
              CDN_ERR_ARG, "null pointer");                                                                                  \
  const CocoAcc a{keys_sorted, perm, dtm, dtig, rank, gt_nonign, rec_thrs, flag, precision, recall, flag_out};

extern "C" int cdn_eval_accumulate_coco(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                        int64_t classes, const unsigned char *dtm, const unsigned char *dtig, const int32_t *rank,
                                        const int32_t *gt_nonign, const double *rec_thrs, const int32_t *flag, double *precision,
                                        double *recall, double *flag_out, void *stream) {
  CDN_EVAL_COCO_ACC_ARGS
  eval_accumulate_coco_kernel<<<dim3((unsigned)classes, E::kAreas * E::kMaxDetsN, E::kThr), kThreads, 0, cdn::as_stream(stream)>>>(t, a);
  return cdn::check_launch("eval accumulate coco");
}
extern "C" int cdn_eval_accumulate_coco_host(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                             int64_t classes, const unsigned char *dtm, const unsigned char *dtig,
                                             const int32_t *rank, const int32_t *gt_nonign, const double *rec_thrs,
                                             const int32_t *flag, double *precision, double *recall, double *flag_out) {
  CDN_EVAL_COCO_ACC_ARGS
  accumulate_coco_host(t, a);
  return CDN_OK;
}
