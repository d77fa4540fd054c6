// codenet_merge.hip -- what CtdetDetector.run does AFTER ctdet_decode for a multi-scale / --nms test (SURVEY.md section 2
// row 22): ctdet_post_process (lib/utils/post_process.py:86-103, lib/detectors/ctdet.py:48-57), the per-class regrouping
// across test scales, soft_nms (lib/models/external/nms.pyx:77-170) and the max_per_image cut of merge_outputs
// (lib/detectors/ctdet.py:59-74), as ONE kernel with one workgroup per image, plus the same soft-NMS on the host
// (cdn_soft_nms_host: no HIP call).  Both call snms_decay() below: one source of arithmetic, tested on the CPU against a
// fixture of the compiled reference (tests/golden/soft_nms_ref.npz) and on the GPU against the host path.
//
// ---- arithmetic ------------------------------------------------------------------------------------------------------
// The widths are those of the C code Cython generates from nms.pyx, not those the .pyx text suggests: the integer literal
// `1` becomes the double 1.0, so every `+ 1` is a double addition.  f() = round to float32, everything else double:
//     area  = f( ((double)f(x2-x1) + 1.0) * ((double)f(y2-y1) + 1.0) )
//     iw    = f( (double)f(min(tx2,x2) - max(tx1,x1)) + 1.0 )        ih likewise;  nothing happens unless iw > 0 and ih > 0
//     ua    = f( ((double)f(tx2-tx1)+1.0) * ((double)f(ty2-ty1)+1.0) + (double)area - (double)f(iw*ih) )
//     ov    = f( f(iw*ih) / ua )
//     w     = method 1: ov > Nt ? f(1.0 - (double)ov) : 1       method 0: ov > Nt ? 0 : 1
//             method 2: f( exp( (double) f( f(-(ov*ov)) / sigma ) ) )      (the double exp)
//     score = f(w * score);   the row is discarded when score < threshold (a float compare)
// No contraction anywhere (hipcc contracts by default: #pragma clang fp contract(off)), divisions correctly rounded.
//
// ---- the state the reference leaves behind ---------------------------------------------------------------------------
// The reference discards a row by overwriting it with row N-1, decrementing N and examining the same position again.  The
// row beyond the new N is NOT cleared, and merge_outputs ignores the returned `keep`: it keeps the whole array, so the
// stale tail rows [N, n) take part in the max_per_image cut and can reach results.json.  This port reproduces that state,
// tail included (reference-faithful, as everywhere else).  What a tail slot holds follows from the loop:
//   * a row that was PULLED (it sat at N-1 when a row further left was discarded) leaves its old slot untouched: box and
//     PRE-decay score of that step (it is decayed only once it is examined in its new slot);
//   * a row discarded IN PLACE (position == N-1: it is overwritten with itself) keeps its DECAYED score.
//
// ---- the kernel ------------------------------------------------------------------------------------------------------
// One workgroup (1024 threads = 16 waves) per image; no cross-workgroup synchronisation, no spinning; every loop is
// bounded by R = S * K.  LDS per workgroup: the class lists [R][5] floats (20 B per row; every decoded row belongs to at
// most one class, so all lists together hold at most R rows), one float of scratch per row (class ids while the rows are
// regrouped, then the pre-decay scores of the current step) and 64 ballot words per wave:
//     24 * R + 16 * 64 * 8 bytes;   R <= kMaxRows = 4096  ->  98304 + 8192 = 106496 bytes of the 160 KiB
//   1. every thread transforms its rows (transform_preds / post_process arithmetic, double then float32) and places them
//      by a STABLE partition by class: the order inside a class is (scale, decode rank), the order np.concatenate gives
//      the reference -- it decides ties and the layout of the tail.  Rank = count of earlier rows of the same class.
//   2. one wave per class, striding over the classes.  Per outer step: wave-wide argmax over [i, N) (strict <, the lowest
//      index wins among equals: per-lane scan in ascending order + a shuffle tree on (score, index)), the swap, then all
//      lanes decay the rows (i, N) in parallel.  Every row of (i, N) is examined exactly once per step whatever the
//      discard order, so the decayed scores and the `bad` flags (examined and below threshold) do not depend on it:
//      they are written in place, the pre-decay scores go to the scratch.  A ballot over the flags commits the step when
//      nobody falls below the threshold (the fast path: nothing more to do).  Otherwise lane 0 replays the reference's
//      discard sequence from the first bad row on -- flags and values are known, so this is a two-pointer walk that only
//      moves rows -- and all lanes restore the pre-decay scores of the tail slots.  (The single-lane fix-up is kept:
//      DESIGN.md section "Multi-scale merge" has the measurement.)
//   3. after a workgroup barrier: thresh = the max_per_image-th largest score over ALL rows of the image, tails included
//      (a rank count over at most R scores; np.partition(scores, kth)[kth]); rows with score >= thresh survive in order
//      (ties may keep more than max_per_image) and are compacted to the front of the output by ballot prefix sums.
#include "cdn_common.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int kMaxRows = 4096;        // S * K per image
constexpr int kMaxClasses = 256;
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaskWords = kMaxRows / 64;

__host__ __device__ __forceinline__ float snms_min(float a, float b) { return a <= b ? a : b; }   // nms.pyx:18-22
__host__ __device__ __forceinline__ float snms_max(float a, float b) { return a >= b ? a : b; }

// One examination of the inner loop (nms.pyx:127-154): the row (x1, y1, x2, y2, s) against the step's maximum t.
// Returns false when the boxes do not overlap (the reference then neither writes the score nor tests the threshold),
// else true with *out = the decayed score.
__host__ __device__ __forceinline__ bool snms_decay(float tx1, float ty1, float tx2, float ty2, float x1, float y1,
                                                    float x2, float y2, float s, float sigma, float Nt, int method,
                                                    float *out) {
#pragma clang fp contract(off)
  const float dw = snms_min(tx2, x2) - snms_max(tx1, x1);
  const float iw = (float)((double)dw + 1.0);
  if (!(iw > 0.0f)) return false;
  const float dh = snms_min(ty2, y2) - snms_max(ty1, y1);
  const float ih = (float)((double)dh + 1.0);
  if (!(ih > 0.0f)) return false;
  const float bw = x2 - x1, bh = y2 - y1;
  const float area = (float)(((double)bw + 1.0) * ((double)bh + 1.0));
  const float tw = tx2 - tx1, th = ty2 - ty1;
  const float inter = iw * ih;
  const double tarea = ((double)tw + 1.0) * ((double)th + 1.0);
  const double usum = tarea + (double)area;
  const float ua = (float)(usum - (double)inter);
#if defined(__HIP_DEVICE_COMPILE__)
  const float ov = __fdiv_rn(inter, ua);
#else
  const float ov = inter / ua;
#endif
  float w;
  if (method == 1) {
    w = ov > Nt ? (float)(1.0 - (double)ov) : 1.0f;
  } else if (method == 2) {
    const float sq = ov * ov;
#if defined(__HIP_DEVICE_COMPILE__)
    const float e = __fdiv_rn(-sq, sigma);
#else
    const float e = -sq / sigma;
#endif
    w = (float)exp((double)e);
  } else {
    w = ov > Nt ? 0.0f : 1.0f;
  }
  *out = w * s;
  return true;
}

// The reference loop, statement by statement, on [n][5] rows in place; returns the final N (= len(keep)).
int64_t soft_nms_rows(float *b, int64_t n, float sigma, float Nt, float threshold, int method) {
  int64_t N = n;
  for (int64_t i = 0; i < N; ++i) {       // (range(N) is evaluated once, but steps at i >= N do nothing)
    float maxscore = b[i * 5 + 4];
    int64_t maxpos = i;
    for (int64_t pos = i + 1; pos < N; ++pos)
      if (maxscore < b[pos * 5 + 4]) {
        maxscore = b[pos * 5 + 4];
        maxpos = pos;
      }
    float t[5];
    std::memcpy(t, b + i * 5, sizeof t);
    std::memcpy(b + i * 5, b + maxpos * 5, sizeof t);
    std::memcpy(b + maxpos * 5, t, sizeof t);
    const float tx1 = b[i * 5], ty1 = b[i * 5 + 1], tx2 = b[i * 5 + 2], ty2 = b[i * 5 + 3];
    int64_t pos = i + 1;
    while (pos < N) {
      float *r = b + pos * 5;
      float ns;
      if (snms_decay(tx1, ty1, tx2, ty2, r[0], r[1], r[2], r[3], r[4], sigma, Nt, method, &ns)) {
        r[4] = ns;
        if (ns < threshold) {
          std::memmove(r, b + (N - 1) * 5, sizeof t);      // pos == N - 1: onto itself (keeps the decayed score)
          --N;
          --pos;
        }
      }
      ++pos;
    }
  }
  return N;
}

#if defined(__HIPCC__)
// Wave-level ordering of LDS traffic between lanes: DS operations of one wave execute in program order; this keeps the
// compiler from moving them across the point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// soft-NMS of one class list by one wave.  L: [n][5] rows in LDS, pre: [n] floats of scratch, wm: kMaskWords ballot
// words of this wave.  Returns the final N.
__device__ int wave_soft_nms(float *L, float *pre, unsigned long long *wm, int n, float sigma, float Nt, float threshold,
                             int method) {
  const int lane = threadIdx.x & 63;
  int N = n;
  for (int i = 0; i + 1 < N; ++i) {        // (the step at i == N - 1 has nothing behind it)
    // ---- argmax over [i, N): first index that attains the maximum --------------------------------------------------
    float best = 0.0f;
    int bi = 0x7fffffff;
    for (int r = i + lane; r < N; r += 64) {
      const float s = L[r * 5 + 4];
      if (bi == 0x7fffffff || best < s) {
        best = s;
        bi = r;
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const float ob = __shfl_xor(best, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || best < ob || (best == ob && oi < bi))) {
        best = ob;
        bi = oi;
      }
    }
    // ---- swap rows i and bi ------------------------------------------------------------------------------------------
    if (bi != i && lane < 5) {
      const float a = L[i * 5 + lane], c = L[bi * 5 + lane];
      L[i * 5 + lane] = c;
      L[bi * 5 + lane] = a;
    }
    wave_sync();
    const float tx1 = L[i * 5], ty1 = L[i * 5 + 1], tx2 = L[i * 5 + 2], ty2 = L[i * 5 + 3];
    // ---- decay (i, N): new scores in place, pre-decay scores to the scratch, `bad` ballots -----------------------------
    const int base = i + 1;
    int first_bad = -1;
    for (int c0 = base; c0 < N; c0 += 64) {
      const int r = c0 + lane;
      bool bad = false;
      if (r < N) {
        const float s = L[r * 5 + 4];
        float ns;
        pre[r] = s;
        if (snms_decay(tx1, ty1, tx2, ty2, L[r * 5], L[r * 5 + 1], L[r * 5 + 2], L[r * 5 + 3], s, sigma, Nt, method,
                       &ns)) {
          L[r * 5 + 4] = ns;
          bad = ns < threshold;
        }
      }
      const unsigned long long mask = __ballot(bad);
      if (lane == 0) wm[(c0 - base) >> 6] = mask;
      if (first_bad < 0 && mask) first_bad = c0 + (int)__ffsll((long long)mask) - 1;
    }
    if (first_bad < 0) continue;            // fast path: nobody fell below the threshold, the step is committed
    wave_sync();
    // ---- discards: lane 0 replays the reference's sequence (values and flags are known: it only moves rows) -----------
    // `cur` = the row that occupies slot `pos` right now: the slot's own, or the one pulled from the right end (slots on
    // the right are never written before they are pulled, so row index == slot there).
    int Nf = 0, inplace = 0;
    if (lane == 0) {
      int pos = first_bad, Nn = N, cur = first_bad;
      while (pos < Nn) {
        const int k = cur - base;
        if ((wm[k >> 6] >> (k & 63)) & 1ull) {
          if (pos == Nn - 1) {              // discarded in place: the slot keeps its occupant with the DECAYED score
            if (cur != pos)
              for (int q = 0; q < 5; ++q) L[pos * 5 + q] = L[cur * 5 + q];
            inplace = 1;
            --Nn;
          } else {                          // overwritten by row N - 1, examined next in this slot
            cur = Nn - 1;
            --Nn;
          }
        } else {
          if (cur != pos)
            for (int q = 0; q < 5; ++q) L[pos * 5 + q] = L[cur * 5 + q];
          ++pos;
          cur = pos;
        }
      }
      Nf = Nn;
    }
    Nf = __shfl(Nf, 0, 64);
    inplace = __shfl(inplace, 0, 64);
    wave_sync();
    // the slots behind the new N hold what was there BEFORE this step's decay (they were pulled, not examined in place)
    for (int r = Nf + inplace + lane; r < N; r += 64) L[r * 5 + 4] = pre[r];
    wave_sync();
    N = Nf;
  }
  return N;
}

__global__ void __launch_bounds__(kThreads)
merge_scales_kernel(const float *__restrict__ dets, const double *__restrict__ meta, int S, int K, int C,
                    int max_per_image, int do_nms, float sigma, float Nt, float threshold, int method,
                    float *__restrict__ boxes, int *__restrict__ rows_out, int *__restrict__ rows_in,
                    int *__restrict__ live, float *__restrict__ thresh_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int cnt[kMaxClasses];
  __shared__ int off[kMaxClasses + 1];
  __shared__ float s_thresh;
  const int R = S * K, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long *wmask = reinterpret_cast<unsigned long long *>(smem);            // [kWaves][kMaskWords]
  float *lists = reinterpret_cast<float *>(smem + (size_t)kWaves * kMaskWords * 8);     // [R][5]
  float *scr = lists + (size_t)R * 5;                                                   // [R]
  int *scr_i = reinterpret_cast<int *>(scr);
  const float *dp = dets + (size_t)b * R * 6;
  for (int c = tid; c < C; c += kThreads) cnt[c] = 0;
  if (tid == 0) s_thresh = -INFINITY;
  __syncthreads();
  // ---- 1. class of every row (a row whose class is not one of 0 .. C-1 belongs to no list, as on the host) ------------
  for (int r = tid; r < R; r += kThreads) {
    const float cf = dp[r * 6 + 5];
    int cls = -1;
    if (cf >= 0.0f && cf < (float)C) {
      cls = (int)cf;
      if ((float)cls != cf) cls = -1;
    }
    scr_i[r] = cls;
    if (cls >= 0) atomicAdd(&cnt[cls], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < C; ++c) {
      off[c] = acc;
      acc += cnt[c];
    }
    off[C] = acc;
  }
  __syncthreads();
  // ---- stable partition + ctdet_post_process -------------------------------------------------------------------------
  for (int r = tid; r < R; r += kThreads) {
    const int cls = scr_i[r];
    if (cls < 0) continue;
    int rank = 0;
#pragma unroll 8
    for (int q = 0; q < r; ++q) rank += scr_i[q] == cls ? 1 : 0;
    const int s = r / K;
    const double *m = meta + ((size_t)b * S + s) * 6;
    float *o = lists + (size_t)(off[cls] + rank) * 5;
    {
#pragma clang fp contract(off)
      const double k = m[2] / m[3], hx = m[3] * 0.5, hy = m[4] * 0.5;
      const float sc = (float)m[5];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double p = (double)dp[r * 6 + q];
        const double t = (q & 1) ? (p - hy) * k : (p - hx) * k;
        const float v = (float)(t + ((q & 1) ? m[1] : m[0]));
        o[q] = __fdiv_rn(v, sc);
      }
    }
    o[4] = dp[r * 6 + 4];
  }
  __syncthreads();
  // ---- 2. soft-NMS: one wave per class ---------------------------------------------------------------------------------
  for (int c = wave; c < C; c += kWaves) {
    const int n = cnt[c];
    int N = n;
    if (do_nms && n > 0)
      N = wave_soft_nms(lists + (size_t)off[c] * 5, scr + off[c], wmask + (size_t)wave * kMaskWords, n, sigma, Nt,
                        threshold, method);
    if (lane == 0) {
      rows_in[(size_t)b * C + c] = n;
      live[(size_t)b * C + c] = N;
    }
  }
  __syncthreads();
  // ---- 3. the cut: the max_per_image-th largest score over all rows (the lists are contiguous: rows [0, T)) ------------
  const int T = off[C];
  const bool cut = T > max_per_image;
  if (cut) {
    for (int r = tid; r < T; r += kThreads) {
      const float s = lists[r * 5 + 4];
      int gt = 0, ge = 0;
#pragma unroll 4
      for (int q = 0; q < T; ++q) {
        const float o = lists[q * 5 + 4];
        gt += o > s ? 1 : 0;
        ge += o >= s ? 1 : 0;
      }
      if (gt < max_per_image && ge >= max_per_image) s_thresh = s;     // (every writer holds the same value)
    }
  }
  __syncthreads();
  const float th = s_thresh;
  if (tid == 0) thresh_out[b] = th;
  for (int c = wave; c < C; c += kWaves) {
    const int n = cnt[c];
    const float *L = lists + (size_t)off[c] * 5;
    float *ob = boxes + ((size_t)b * C + c) * (size_t)R * 5;
    int count = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int r = c0 + lane;
      const bool keep = r < n && (!cut || L[r * 5 + 4] >= th);
      const unsigned long long mask = __ballot(keep);
      if (keep) {
        const int p = count + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
        for (int q = 0; q < 5; ++q) ob[(size_t)p * 5 + q] = L[r * 5 + q];
      }
      count += __popcll(mask);
    }
    if (lane == 0) rows_out[(size_t)b * C + c] = count;
  }
}
#endif

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

int check_snms_args(float sigma, int method) {
  CDN_REQUIRE(method >= 0 && method <= 2, CDN_ERR_ARG, "soft-NMS method %d (0 hard, 1 linear, 2 gaussian)", method);
  CDN_REQUIRE(method != 2 || sigma != 0.0f, CDN_ERR_ARG, "gaussian soft-NMS needs sigma != 0");
  return CDN_OK;
}

}  // namespace

extern "C" int cdn_soft_nms_host(float *boxes, int64_t n, float sigma, float Nt, float threshold, int method,
                                 int64_t *n_keep) {
  CDN_REQUIRE(n >= 0 && (boxes || n == 0), CDN_ERR_ARG, "null pointer or negative row count");
  const int rc = check_snms_args(sigma, method);
  if (rc) return rc;
  const int64_t N = n ? soft_nms_rows(boxes, n, sigma, Nt, threshold, method) : 0;
  if (n_keep) *n_keep = N;
  return CDN_OK;
}

extern "C" size_t cdn_ctdet_merge_scales_workspace_bytes(int64_t B, int64_t S, int64_t K, int64_t num_classes) {
  if (B <= 0 || S <= 0 || K <= 0 || num_classes <= 0) return 0;
  return round256((size_t)(B * num_classes * S * K) * 5 * 4) + 3 * round256((size_t)(B * num_classes) * 4) +
         round256((size_t)B * 4);
}

extern "C" int cdn_ctdet_merge_scales(const float *dets, const double *meta, int64_t B, int64_t S, int64_t K,
                                      int64_t num_classes, int max_per_image, int do_nms, float sigma, float Nt,
                                      float threshold, int method, float *boxes, int32_t *rows_out, int32_t *rows_in,
                                      int32_t *live, float *thresh, void *stream) {
  CDN_REQUIRE(dets && meta && boxes && rows_out && rows_in && live && thresh, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(B > 0 && S > 0 && K > 0 && num_classes > 0 && max_per_image > 0, CDN_ERR_ARG, "non-positive size");
  const int rc = check_snms_args(sigma, method);
  if (rc) return rc;
  CDN_REQUIRE(K <= 1024, CDN_ERR_UNSUPPORTED, "K = %lld unsupported (cdn_ctdet_decode writes at most 1024)", (long long)K);
  CDN_REQUIRE(S * K <= kMaxRows, CDN_ERR_UNSUPPORTED, "S * K = %lld rows per image exceed the LDS lists (%d)",
              (long long)(S * K), kMaxRows);
  CDN_REQUIRE(num_classes <= kMaxClasses, CDN_ERR_UNSUPPORTED, "more than %d classes", kMaxClasses);
  CDN_REQUIRE(B <= 65535 * 1024, CDN_ERR_UNSUPPORTED, "batch too large");
  const size_t lds = (size_t)kWaves * kMaskWords * 8 + (size_t)(S * K) * 24;
  (void)hipFuncSetAttribute((const void *)merge_scales_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  merge_scales_kernel<<<(unsigned)B, kThreads, lds, cdn::as_stream(stream)>>>(
      dets, meta, (int)S, (int)K, (int)num_classes, max_per_image, do_nms ? 1 : 0, sigma, Nt, threshold, method, boxes,
      rows_out, rows_in, live, thresh);
  return cdn::check_launch("ctdet merge scales");
}
