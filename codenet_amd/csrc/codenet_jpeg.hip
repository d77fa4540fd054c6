// codenet_jpeg.hip -- baseline JPEG decoding in front of the pre-processing: file bytes -> interleaved uint8 pixels, the
// bits of libjpeg-turbo's default decode (what cv2.imread and PIL give).  DESIGN.md section 7.4d is the contract,
// tests/jpeg_ref.py restates it in numpy; the arithmetic, the host half and the decoder core are cdn_jpeg.h, plain C++ that
// the kernels here and cdn_jpeg_decode_host both run.
//
// ---- the kernels -----------------------------------------------------------------------------------------------------
// jpeg_entropy_idct_kernel: one wave per workgroup, a grid that follows from the capacities alone; the waves stride over
//   the segment records, whose count is a word of device memory, so a captured launch replays for any batch inside the
//   capacity.  Per segment the item's 6 KB of quantisation and Huffman tables go to LDS (kept while consecutive segments
//   belong to one item) and the segment's bytes pass through a 2 KB LDS window that all lanes refill between two MCUs;
//   lane 0 decodes the blocks of one MCU (at most 6) into a zeroed LDS tile; then 8 lanes per block
//   run the column pass and the row pass through LDS, store each row of 8 samples as one 64-bit word and clear the tile.
//   The Huffman decode of a segment is a dependent chain on ONE lane: the concurrency of this kernel is the number of
//   segments, batch size x restart intervals -- for files without restart markers (Pascal VOC) the batch size.
//   The item status is combined with an integer atomicMax: any order gives the same bits.
// jpeg_color_kernel: a thread per pair of output pixels of an item, grid-stride; fancy up-sampling of Cb / Cr from the
//   planes with the edge rules of the TRUE component size, colour conversion, interleaved byte stores.
#include "cdn_common.h"
#include "cdn_jpeg.h"

namespace {

namespace J = cdn_jpeg;
constexpr int kColorThreads = 256;

struct WaveSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }      // the workgroup is one wave
};

__global__ void __launch_bounds__(64) jpeg_entropy_idct_kernel(J::Call c) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[J::kTableBytes / 4];
  __shared__ int s_tile[6 * 64], s_ws[6 * 64], s_flag[2];
  __shared__ uint8_t s_win[J::kWindow];
  const int lane = threadIdx.x;
  for (int k = lane; k < 6 * 64; k += 64) s_tile[k] = 0;
  int loaded = -1;
  const int ns = J::n_segments(c), ni = J::n_items(c);
  for (int s = blockIdx.x; s < ns; s += gridDim.x) {
    J::Segment sg;
    if (!J::segment_geom(c, s, &sg)) {          // (the same answer in every lane)
      const int item = c.segs[(int64_t)(1 + s) * J::kSegWords + J::kSegItem];
      if (lane == 0 && item >= 0 && item < ni) atomicMax(c.status + item, (int)J::kBadRecord);
      continue;
    }
    if (sg.item != loaded) {
      __syncthreads();
      const uint32_t *src = reinterpret_cast<const uint32_t *>(c.tables + (int64_t)sg.item * J::kTableBytes);
      for (int k = lane; k < J::kTableBytes / 4; k += 64) s_tab[k] = src[k];
      loaded = sg.item;
    }
    __syncthreads();
    const int st = J::decode_segment(sg, reinterpret_cast<const J::Tables *>(s_tab), c.planes + sg.item * c.plane_stride,
                                     s_tile, s_ws, s_win, s_flag, lane, 64, WaveSync());
    if (st && lane == 0) atomicMax(c.status + sg.item, st);
  }
}

__global__ void __launch_bounds__(kColorThreads) jpeg_color_kernel(J::Call c) {
  const int item = blockIdx.y;
  if (item >= J::n_items(c)) return;
  J::Geom g;
  if (!J::item_geom(c.items + (int64_t)item * J::kItemWords, c.plane_stride, &g) || !J::out_fits(g, c.out_cap)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(c.status + item, (int)J::kBadRecord);
    return;
  }
  const uint8_t *planes = c.planes + item * c.plane_stride;
  const int pw = (g.w + 1) / 2;
  const int64_t npairs = (int64_t)pw * g.h;
  for (int64_t p = (int64_t)blockIdx.x * kColorThreads + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * kColorThreads) {
    const int y = (int)(p / pw), i = (int)(p - (int64_t)y * pw);
    J::color_pair(g, planes, c.out, y, i, c.rgb);
  }
}

// ---- the parallel entropy path (cdn_jpeg_decode_parallel): three launches --------------------------------------------------
// jpeg_entropy_parallel_kernel: a workgroup of W = 256 lanes per segment, striding over the records like the kernel above.
//   The segment's bits are cut into sub-sequences of subseq_bits, 256 to a tile; the tile's bytes go to an LDS window and
//   J::decode_segment_parallel runs the dry pass, the counted synchronisation rounds, the prefix sum and the write pass
//   on them; raw coefficients and DC words go to the item's workspace.  Every barrier is reached by every lane.
// jpeg_idct_kernel: all blocks of all items, 32 to a workgroup step (8 lanes a block), grid-stride with a grid from the
//   capacities: dequantise, the two IDCT passes through LDS, rows of 8 samples to the planes.
// jpeg_color_kernel, unchanged.
constexpr int kIdctBlocks = 32;     // blocks per workgroup step of jpeg_idct_kernel

struct GroupSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }      // the four waves of the workgroup
};

__global__ void __launch_bounds__(J::kParLanes) jpeg_entropy_parallel_kernel(J::ParCall pc) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[J::kTableBytes / 4];
  __shared__ J::PState s_exit[2 * J::kParLanes], s_entry[J::kParLanes];
  __shared__ int s_cnt[J::kParLanes], s_flag[3];
  __shared__ uint32_t s_scan[4 * J::kParLanes];
  __shared__ uint8_t s_win[J::kParWindow];
  const J::Call &c = pc.c;
  const J::ParShared sh{s_exit, s_entry, s_cnt, s_scan, s_flag, s_win};
  const int lane = threadIdx.x;
  int loaded = -1;
  const int ns = J::n_segments(c), ni = J::n_items(c);
  for (int s = blockIdx.x; s < ns; s += gridDim.x) {
    J::Segment sg;
    if (!J::segment_geom(c, s, &sg)) {          // (the same answer in every lane)
      const int item = c.segs[(int64_t)(1 + s) * J::kSegWords + J::kSegItem];
      if (lane == 0 && item >= 0 && item < ni) atomicMax(c.status + item, (int)J::kBadRecord);
      continue;
    }
    if (sg.item != loaded) {
      __syncthreads();
      const uint32_t *src = reinterpret_cast<const uint32_t *>(c.tables + (int64_t)sg.item * J::kTableBytes);
      for (int k = lane; k < J::kTableBytes / 4; k += J::kParLanes) s_tab[k] = src[k];
      loaded = sg.item;
    }
    __syncthreads();
    const int st = J::decode_segment_parallel(sg, reinterpret_cast<const J::Tables *>(s_tab), J::par_coef(pc, sg.item),
                                              J::par_dc(pc, sg.item), pc.subseq_bits, sh, lane, J::kParLanes, GroupSync());
    if (st && lane == 0) atomicMax(c.status + sg.item, st);
  }
}

__global__ void __launch_bounds__(kIdctBlocks * 8) jpeg_idct_kernel(J::ParCall pc) {
  __shared__ int s_tile[kIdctBlocks * 64], s_ws[kIdctBlocks * 64];
  const J::Call &c = pc.c;
  const int64_t steps_per_item = (J::par_blocks(c.plane_stride) + kIdctBlocks - 1) / kIdctBlocks;
  const int64_t steps = steps_per_item * J::n_items(c);
  const int lb = threadIdx.x >> 3, l = threadIdx.x & 7;
  for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {      // (item, geometry and `first`: the same in every lane)
    const int item = (int)(step / steps_per_item);
    const int64_t first = (step - item * steps_per_item) * kIdctBlocks;
    J::Geom g;
    if (!J::item_geom(c.items + (int64_t)item * J::kItemWords, c.plane_stride, &g)) continue;      // (the colour kernel flags it)
    const int nblk = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    const int64_t total = (int64_t)g.mcus_x * g.mcus_y * nblk;
    if (first >= total) continue;
    const int64_t blk = first + lb;
    const bool valid = blk < total;
    const int mi = (int)(blk / nblk), b = (int)(blk - (int64_t)mi * nblk), my = mi / g.mcus_x, mx = mi - my * g.mcus_x;
    int *tile = s_tile + lb * 64, *ws = s_ws + lb * 64;
    if (valid) {
      const J::Tables *tab = reinterpret_cast<const J::Tables *>(c.tables + (int64_t)item * J::kTableBytes);
      J::par_dequant_row(J::par_coef(pc, item), J::par_dc(pc, item), blk, tab->quant[J::block_comp(g, b)], l, tile);
    }
    __syncthreads();
    if (valid) J::idct_column(tile, ws, l);
    __syncthreads();
    if (valid) {
      int comp, pitch;
      uint8_t *o = J::block_origin(g, c.planes + item * c.plane_stride, mx, my, b, &comp, &pitch);
      J::store8(o + (int64_t)l * pitch, J::idct_row(ws, l));
    }
  }
}

int make_call(J::Call *c,const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
              const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
              int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb) {
  CDN_REQUIRE(stream_bytes && segs && items && tables && planes && status && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(stream_cap > 0 && seg_cap > 0 && item_cap > 0 && plane_stride > 0 && out_cap > 0, CDN_ERR_ARG,
              "non-positive capacity");
  CDN_REQUIRE(stream_cap <= 0x7fffffff, CDN_ERR_UNSUPPORTED, "stream capacity beyond 2^31 - 1 bytes");
  CDN_REQUIRE(item_cap <= 65535 && seg_cap <= 0x7fffffff / J::kSegWords - 1, CDN_ERR_UNSUPPORTED,
              "more than 65535 items or 2^28 segments");
  CDN_REQUIRE(plane_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(planes) & 7) == 0, CDN_ERR_ARG,
              "planes and their stride must be multiples of 8 bytes");
  CDN_REQUIRE(cdn::aligned16(tables) && (reinterpret_cast<uintptr_t>(segs) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(items) & 3) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
              CDN_ERR_ARG, "misaligned table, record or status pointer");
  *c = J::Call{stream_bytes, stream_cap, segs, seg_cap, items, item_cap, tables, planes, plane_stride, status, out, out_cap,
               rgb ? 1 : 0};
  return CDN_OK;
}

int host_result(int rc, const char *msg) { return rc == 0 ? CDN_OK : cdn::fail(rc, "%s", msg); }

}  // namespace

extern "C" int cdn_jpeg_parse(const unsigned char *data, int64_t n, int32_t *info) {
  CDN_REQUIRE(data && info, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(n > 0, CDN_ERR_ARG, "no data");
  J::Header hd;
  char msg[200];
  const int rc = J::parse(data, n, &hd, msg, sizeof(msg));
  if (rc) return host_result(rc, msg);
  const int32_t v[16] = {hd.w, hd.h, hd.ncomp, hd.mode, hd.mcus_x, hd.mcus_y, hd.restart, hd.n_segments,
                         (int32_t)(hd.scan_off & 0x7fffffff), 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 16; ++k) info[k] = v[k];
  return CDN_OK;
}

extern "C" size_t cdn_jpeg_workspace_bytes(int64_t max_items, int64_t max_h, int64_t max_w) {
  if (max_items < 1 || max_h < 1 || max_w < 1 || max_h > 65535 || max_w > 65535) return 0;
  return (size_t)max_items * (size_t)J::plane_stride(max_h, max_w);
}

extern "C" int cdn_jpeg_pack(const unsigned char *data, int64_t n, int32_t item, int64_t out_off, int64_t out_pitch,
                             unsigned char *stream_bytes, int64_t stream_used, int64_t stream_cap, int32_t *segs,
                             int64_t segs_used, int64_t seg_cap, int32_t *item_rec, unsigned char *tables,
                             int64_t plane_stride, int64_t *used) {
  CDN_REQUIRE(data && stream_bytes && segs && item_rec && tables && used, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(n > 0 && item >= 0 && item < 65535, CDN_ERR_ARG, "no data or item index outside 0..65534");
  CDN_REQUIRE(stream_used >= 0 && stream_used <= stream_cap && segs_used >= 0 && segs_used <= seg_cap && plane_stride > 0,
              CDN_ERR_ARG, "used counts outside the capacities");
  CDN_REQUIRE(cdn::aligned16(tables), CDN_ERR_ARG, "misaligned table blob");
  J::PackTarget tg{stream_bytes, stream_used, stream_cap, segs, segs_used, seg_cap, item_rec, tables, plane_stride};
  char msg[200];
  const int rc = J::pack(data, n, item, out_off, out_pitch, &tg, msg, sizeof(msg));
  if (rc) return host_result(rc, msg);
  used[0] = tg.stream_used;
  used[1] = tg.segs_used;
  return CDN_OK;
}

extern "C" int cdn_jpeg_decode_host(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs,
                                    int64_t seg_cap, const int32_t *items, int64_t item_cap, const unsigned char *tables,
                                    unsigned char *planes, int64_t plane_stride, int32_t *status, unsigned char *out,
                                    int64_t out_cap, int rgb) {
  J::Call c;
  const int rc = make_call(&c, stream_bytes, stream_cap, segs, seg_cap, items, item_cap, tables, planes, plane_stride, status,
                           out, out_cap, rgb);
  if (rc != CDN_OK) return rc;
  J::decode_host(c);
  return CDN_OK;
}

extern "C" int cdn_jpeg_decode(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
                               const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
                               int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb,
                               void *stream) {
  J::Call c;
  const int rc = make_call(&c, stream_bytes, stream_cap, segs, seg_cap, items, item_cap, tables, planes, plane_stride, status,
                           out, out_cap, rgb);
  if (rc != CDN_OK) return rc;
  hipStream_t st = cdn::as_stream(stream);
  // both grids from the capacities: the counts of this batch are device words
  const unsigned eg = (unsigned)(seg_cap < 4096 ? seg_cap : 4096);
  jpeg_entropy_idct_kernel<<<eg, 64, 0, st>>>(c);
  const int re = cdn::check_launch("jpeg entropy_idct");
  if (re != CDN_OK) return re;
  const int64_t cap_pairs = plane_stride / 6;                     // pixel pairs of the largest item the planes hold
  int64_t gx = cdn::ceil_div(cap_pairs, kColorThreads);
  gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
  jpeg_color_kernel<<<dim3((unsigned)gx, (unsigned)item_cap), kColorThreads, 0, st>>>(c);
  return cdn::check_launch("jpeg color");
}

// ---- the parallel entropy path ---------------------------------------------------------------------------------------------
namespace {

int make_par_call(J::ParCall *pc, unsigned char *workspace, size_t workspace_bytes, int subseq_bits) {
  CDN_REQUIRE(workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(J::subseq_bits_ok(subseq_bits), CDN_ERR_ARG, "subseq_bits must be a multiple of 32 in 64..8192, got %d",
              subseq_bits);
  const int64_t stride = J::par_work_stride(pc->c.plane_stride);
  CDN_REQUIRE(stride > 0, CDN_ERR_ARG, "a plane stride below the 64 bytes of one block");
  CDN_REQUIRE(cdn::aligned16(workspace) &&workspace_bytes / (size_t)stride >= (size_t)pc->c.item_cap, CDN_ERR_ARG,
              "the coefficient workspace must be 16-byte aligned and hold %lld bytes per item", (long long)stride);
  pc->work = workspace;
  pc->work_stride = stride;
  pc->subseq_bits = subseq_bits;
  return CDN_OK;
}

}  // namespace

extern "C" size_t cdn_jpeg_parallel_workspace_bytes(int64_t max_items, int64_t max_h, int64_t max_w) {
  if (max_items < 1 || max_h < 1 || max_w < 1 || max_h > 65535 || max_w > 65535) return 0;
  return (size_t)max_items * (size_t)J::par_work_stride(J::plane_stride(max_h, max_w));
}

extern "C" int cdn_jpeg_decode_parallel_host(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs,
                                             int64_t seg_cap, const int32_t *items, int64_t item_cap,
                                             const unsigned char *tables, unsigned char *planes, int64_t plane_stride,
                                             int32_t *status, unsigned char *out, int64_t out_cap, int rgb,
                                             unsigned char *workspace, size_t workspace_bytes, int subseq_bits) {
  J::ParCall pc;
  int rc = make_call(&pc.c, stream_bytes, stream_cap, segs, seg_cap, items, item_cap, tables, planes, plane_stride, status, out,
                     out_cap, rgb);
  if (rc != CDN_OK) return rc;
  rc = make_par_call(&pc, workspace, workspace_bytes, subseq_bits);
  if (rc != CDN_OK) return rc;
  J::decode_host_parallel(pc);
  return CDN_OK;
}

extern "C" int cdn_jpeg_decode_parallel(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs,
                                        int64_t seg_cap, const int32_t *items, int64_t item_cap, const unsigned char *tables,
                                        unsigned char *planes, int64_t plane_stride, int32_t *status, unsigned char *out,
                                        int64_t out_cap, int rgb, unsigned char *workspace, size_t workspace_bytes,
                                        int subseq_bits, void *stream) {
  J::ParCall pc;
  int rc = make_call(&pc.c, stream_bytes, stream_cap, segs, seg_cap, items, item_cap, tables, planes, plane_stride, status, out,
                     out_cap, rgb);
  if (rc != CDN_OK) return rc;
  rc = make_par_call(&pc, workspace, workspace_bytes, subseq_bits);
  if (rc != CDN_OK) return rc;
  hipStream_t st = cdn::as_stream(stream);
  // the three grids from the capacities: the counts of this batch are device words
  const unsigned eg = (unsigned)(seg_cap < 4096 ? seg_cap : 4096);
  jpeg_entropy_parallel_kernel<<<eg, J::kParLanes, 0, st>>>(pc);
  rc = cdn::check_launch("jpeg entropy_parallel");
  if (rc != CDN_OK) return rc;
  int64_t ig = cdn::ceil_div(J::par_blocks(plane_stride), kIdctBlocks) * item_cap;
  ig = ig < 1 ? 1 : (ig > 16384 ? 16384 : ig);
  jpeg_idct_kernel<<<(unsigned)ig, kIdctBlocks * 8, 0, st>>>(pc);
  rc = cdn::check_launch("jpeg idct");
  if (rc != CDN_OK) return rc;
  const int64_t cap_pairs = plane_stride / 6;                     // pixel pairs of the largest item the planes hold
  int64_t gx = cdn::ceil_div(cap_pairs, kColorThreads);
  gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
  jpeg_color_kernel<<<dim3((unsigned)gx, (unsigned)item_cap), kColorThreads, 0, st>>>(pc.c);
  return cdn::check_launch("jpeg color");
}
