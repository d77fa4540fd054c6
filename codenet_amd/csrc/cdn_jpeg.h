// cdn_jpeg.h -- baseline JPEG decoding (DESIGN.md section 7.4d is the contract; tests/jpeg_ref.py restates it in numpy).
// Plain C++ with no HIP call: the host half (header parse, byte packing, decode tables) and the decoder core (bit reader,
// Huffman lookup, one MCU's blocks, the two IDCT passes, fancy up-sampling and colour).  The core is __host__ __device__
// under hipcc: jpeg_entropy_idct_kernel / jpeg_color_kernel (codenet_jpeg.hip) and cdn_jpeg_decode_host run the SAME
// text, the kernel with 64 lanes and a barrier, the host with one lane and none.  The parallel entropy path
// (decode_segment_parallel: a segment on the 256 lanes of a workgroup; jpeg_entropy_parallel_kernel / jpeg_idct_kernel and
// cdn_jpeg_decode_parallel_host) follows the same rule.  tools/probes/jpeg_host_fuzz.cpp includes this file alone.
//
// The target is equality with libjpeg-turbo's default decode (ISLOW IDCT, fancy up-sampling, 16-bit fixed-point colour).
// Everything is integer.  Sums and products of the IDCT are formed in uint32_t: for every stream a conforming encoder
// writes they are the int32 values of jidctint.c, and for a corrupt one they wrap instead of overflowing.
//
// Termination and bounds do not depend on the data: the loops are counted (MCUs of a segment, blocks of an MCU, k < 64
// strictly increasing), the bit reader returns zeros beyond the segment's last byte, a code with no entry after 16 bits
// ends the segment, table indices are masked, and segment_geom() / item_geom() check every record against the capacities before
// anything is stored.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#ifdef __HIPCC__
#define CDN_JPEG_HD __host__ __device__ __forceinline__
#else
#define CDN_JPEG_HD inline
#endif

namespace cdn_jpeg {

// ---- records shared by host and device -----------------------------------------------------------------------------------
constexpr int kItemWords = 16;      // int32 per item record
enum ItemWord {
  kW = 0, kH = 1, kNComp = 2, kMode = 3,          // mode: 0 every component 1x1 (4:4:4, grey), 1 Y 2x1 (4:2:2), 2 Y 2x2 (4:2:0)
  kMcusX = 4, kMcusY = 5, kSel = 6,               // sel: bit 2c = DC table of component c, bit 2c + 1 = its AC table
  kPitchY = 7, kRowsY = 8, kPitchC = 9, kRowsC = 10, kRestart = 11,
  kOutLo = 12, kOutHi = 13, kOutPitch = 14        // where the item's interleaved bytes go in the output buffer
};
constexpr int kSegWords = 8;        // int32 per segment record; record 0 is the header {n_segments, n_items}
enum SegWord { kSegItem = 0, kSegFirst = 1, kSegCount = 2, kSegOff = 3, kSegLen = 4 };
enum Status { kOk = 0, kOverread = 1, kBadCode = 2, kBadRecord = 3 };

struct Huff {                       // decode form of one Huffman table
  uint16_t look[512];               // 9-bit look-ahead: (length << 8) | symbol, 0 = longer than 9 bits or no code
  int32_t maxcode[17];              // [l]: largest code of length l, -1 = none
  int32_t valoff[17];               // [l]: index into huffval of the first code of length l, minus that code
  uint8_t huffval[256];
  uint8_t pad[56];
};
struct Tables {                     // the blob of one item: 6144 bytes
  uint8_t quant[3][64];             // per COMPONENT, natural order
  uint8_t zigzag[64];               // natural-order index of zig-zag position k (beside the tables: an LDS read on the device)
  Huff huff[4];                     // DC 0, DC 1, AC 0, AC 1
};
static_assert(sizeof(Huff) == 1472 && sizeof(Tables) == 6144, "table blob layout");
constexpr int kTableBytes = 6144;

// planes of one item: what a max_h x max_w 4:4:4 image needs, padded to whole 16 x 16 MCUs
CDN_JPEG_HD int64_t plane_stride(int64_t max_h, int64_t max_w) {
  const int64_t n = 3 * ((max_h + 15) / 16 * 16) * ((max_w + 15) / 16 * 16);
  return (n + 255) / 256 * 256;
}

// everything a decode call is given; the same struct for device and host pointers
struct Call {
  const uint8_t *stream;
  int64_t stream_cap;
  const int32_t *segs;
  int64_t seg_cap;                  // records behind the header
  const int32_t *items;
  int64_t item_cap;
  const uint8_t *tables;
  uint8_t *planes;
  int64_t plane_stride;
  int32_t *status;
  uint8_t *out;
  int64_t out_cap;
  int rgb;
};

CDN_JPEG_HD int n_segments(const Call &c) {
  const int64_t n = c.segs[0];
  return (int)(n < 0 ? 0 : (n > c.seg_cap ? c.seg_cap : n));
}
CDN_JPEG_HD int n_items(const Call &c) {
  const int64_t n = c.segs[1];
  return (int)(n < 0 ? 0 : (n > c.item_cap ? c.item_cap : n));
}

// geometry of an item, checked against the plane capacity
struct Geom {
  int w, h, ncomp, mode, hs, vs, mcus_x, mcus_y, sel, pitch_y, rows_y, pitch_c, rows_c;
  int64_t out_off, out_pitch;
};
CDN_JPEG_HD bool item_geom(const int32_t *it, int64_t plane_stride_, Geom *g) {
  g->w = it[kW];
  g->h = it[kH];
  g->ncomp = it[kNComp];
  g->mode = it[kMode];
  g->mcus_x = it[kMcusX];
  g->mcus_y = it[kMcusY];
  g->sel = it[kSel];
  g->out_off = (int64_t)(((uint64_t)(uint32_t)it[kOutHi] << 32) | (uint32_t)it[kOutLo]);
  g->out_pitch = it[kOutPitch];
  if (g->w < 1 || g->h < 1 || g->w > 65535 || g->h > 65535 || (g->ncomp != 1 && g->ncomp != 3) || g->mode < 0 ||
      g->mode > 2 || (g->ncomp == 1 && g->mode != 0))
    return false;
  g->hs = g->mode >= 1 ? 2 : 1;
  g->vs = g->mode == 2 ? 2 : 1;
  // the sizes follow from w, h and the mode; the record's copies must agree
  if (g->mcus_x != (g->w + 8 * g->hs - 1) / (8 * g->hs) || g->mcus_y != (g->h + 8 * g->vs - 1) / (8 * g->vs)) return false;
  g->pitch_y = g->mcus_x * 8 * g->hs;
  g->rows_y = g->mcus_y * 8 * g->vs;
  g->pitch_c = g->mcus_x * 8;
  g->rows_c = g->mcus_y * 8;
  if (it[kPitchY] != g->pitch_y || it[kRowsY] != g->rows_y || it[kPitchC] != g->pitch_c || it[kRowsC] != g->rows_c)
    return false;
  const int64_t need = (int64_t)g->pitch_y * g->rows_y + (g->ncomp == 3 ? 2 * (int64_t)g->pitch_c * g->rows_c : 0);
  return need <= plane_stride_;
}
CDN_JPEG_HD bool out_fits(const Geom &g, int64_t out_cap) {
  return g.out_off >= 0 && g.out_pitch >= 3 * (int64_t)g.w &&
         g.out_off + (int64_t)(g.h - 1) * g.out_pitch + 3 * (int64_t)g.w <= out_cap;
}

// a segment record checked against the capacities
struct Segment {
  int item, first, count;
  const uint8_t *bytes;
  int len;
  Geom g;
};
CDN_JPEG_HD bool segment_geom(const Call &c, int s, Segment *sg) {
  const int32_t *r = c.segs + (int64_t)(1 + s) * kSegWords;
  sg->item = r[kSegItem];
  sg->first = r[kSegFirst];
  sg->count = r[kSegCount];
  sg->len = r[kSegLen];
  const int64_t off = r[kSegOff];
  if (sg->item < 0 || sg->item >= n_items(c)) return false;
  if (off < 0 || sg->len < 0 || off + sg->len > c.stream_cap) return false;
  if (!item_geom(c.items + (int64_t)sg->item * kItemWords, c.plane_stride, &sg->g)) return false;
  const int64_t total = (int64_t)sg->g.mcus_x * sg->g.mcus_y;
  if (sg->first < 0 || sg->count < 0 || (int64_t)sg->first + sg->count > total) return false;
  sg->bytes = c.stream + off;
  return true;
}

// ---- bit reader: MSB first over bytes whose stuffing the host removed -----------------------------------------------------
struct Bits {
  const uint8_t *p;
  const uint8_t *win;               // a copy of bytes [wbase, wend) of the segment in fast memory (LDS on the device), or null
  int wbase, wend;
  int len, pos;
  uint64_t acc;       // the next bits in the HIGH end
  int n;              // valid bits in acc (phantom zeros included)
  int real;           // bits of acc that came from the segment; < 0: bits beyond its end were consumed
};
CDN_JPEG_HD void bits_init(Bits *b, const uint8_t *p, int len) {
  b->p = p;
  b->win = nullptr;
  b->wbase = b->wend = 0;
  b->len = len;
  b->pos = 0;
  b->acc = 0;
  b->n = 0;
  b->real = 0;
}
CDN_JPEG_HD uint32_t load_be32(const uint8_t *q) {
  return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
}
// at least 32 bits in acc
CDN_JPEG_HD void bits_fill(Bits *b) {
  if (b->n > 32) return;
  uint32_t v = 0;
  int got = b->len - b->pos;
  if (b->pos >= b->wbase && b->pos + 4 <= b->wend) {      // (two branches: the window is LDS, p global memory)
    v = load_be32(b->win + (b->pos - b->wbase));
    got = 4;
  } else if (got >= 4) {
    v = load_be32(b->p + b->pos);
    got = 4;
  } else {
    for (int i = 0; i < got; ++i) v |= (uint32_t)b->p[b->pos + i] << (24 - 8 * i);
  }
  b->pos += got;
  b->acc |= (uint64_t)v << (32 - b->n);
  b->n += 32;
  b->real += 8 * got;
}
CDN_JPEG_HD uint32_t bits_peek(const Bits *b, int k) { return (uint32_t)(b->acc >> (64 - k)); }      // 1 <= k <= 32
CDN_JPEG_HD void bits_skip(Bits *b, int k) {
  b->acc <<= k;
  b->n -= k;
  b->real -= k;
}

// one Huffman symbol; -1: no code matches the next 16 bits.  At most 16 bits consumed; the caller filled to >= 32.
CDN_JPEG_HD int huff_symbol(Bits *b, const Huff *t) {
  const uint32_t e = t->look[bits_peek(b, 9)];
  if (e) {
    bits_skip(b, (int)(e >> 8) & 15);
    return (int)(e & 255);
  }
  const int32_t code16 = (int32_t)bits_peek(b, 16);
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = code16 >> (16 - l);
    if (code <= t->maxcode[l]) {
      bits_skip(b, l);
      return t->huffval[(code + t->valoff[l]) & 255];
    }
  }
  return -1;
}
// the t-bit value that follows a symbol, sign-extended: extend(v, t) = v if v >= 2^(t-1) else v - 2^t + 1
CDN_JPEG_HD int receive_extend(Bits *b, int t) {
  const int v = (int)bits_peek(b, t);
  bits_skip(b, t);
  return v >= (1 << (t - 1)) ? v : v - (1 << t) + 1;
}

CDN_JPEG_HD int zigzag(int k) {
  // natural-order index of zig-zag position k, 6 bits each in 8-entry words (no table in memory: the same on both sides)
  constexpr uint64_t z[8] = {
      0ull | (1ull << 6) | (8ull << 12) | (16ull << 18) | (9ull << 24) | (2ull << 30) | (3ull << 36) | (10ull << 42),
      17ull | (24ull << 6) | (32ull << 12) | (25ull << 18) | (18ull << 24) | (11ull << 30) | (4ull << 36) | (5ull << 42),
      12ull | (19ull << 6) | (26ull << 12) | (33ull << 18) | (40ull << 24) | (48ull << 30) | (41ull << 36) | (34ull << 42),
      27ull | (20ull << 6) | (13ull << 12) | (6ull << 18) | (7ull << 24) | (14ull << 30) | (21ull << 36) | (28ull << 42),
      35ull | (42ull << 6) | (49ull << 12) | (56ull << 18) | (57ull << 24) | (50ull << 30) | (43ull << 36) | (36ull << 42),
      29ull | (22ull << 6) | (15ull << 12) | (23ull << 18) | (30ull << 24) | (37ull << 30) | (44ull << 36) | (51ull << 42),
      58ull | (59ull << 6) | (52ull << 12) | (45ull << 18) | (38ull << 24) | (31ull << 30) | (39ull << 36) | (46ull << 42),
      53ull | (60ull << 6) | (61ull << 12) | (54ull << 18) | (47ull << 24) | (55ull << 30) | (62ull << 36) | (63ull << 42)};
  return (int)((z[(k >> 3) & 7] >> (6 * (k & 7))) & 63);
}

// One 8 x 8 block: entropy-decode into the ZEROED tile (natural order, dequantised).  -> 0 or kBadCode.
CDN_JPEG_HD int decode_block(Bits *b, const Huff *dc, const Huff *ac, const uint8_t *q, const uint8_t *zz, int *pred,
                             int *tile) {
  bits_fill(b);
  int s = huff_symbol(b, dc);
  if (s < 0) return kBadCode;
  s &= 15;
  int diff = 0;
  if (s) {
    bits_fill(b);
    diff = receive_extend(b, s);
  }
  *pred = (int)((uint32_t)*pred + (uint32_t)diff);
  tile[0] = (int)((uint32_t)*pred * (uint32_t)q[0]);
  for (int k = 1; k < 64;) {          // k grows by at least 1 per iteration
    bits_fill(b);
    const int rs = huff_symbol(b, ac);
    if (rs < 0) return kBadCode;
    const int r = rs >> 4, t = rs & 15;
    if (t) {
      k += r;
      const int v = receive_extend(b, t);        // (<= 16 + 15 bits since the fill)
      if (k < 64) {
        const int n = zz[k] & 63;
        tile[n] = (int)((uint32_t)v * (uint32_t)q[n]);
      }
      k += 1;
    } else if (r == 15) {
      k += 16;                                   // ZRL
    } else {
      break;                                     // EOB
    }
  }
  return 0;
}

// ---- jidctint.c: CONST_BITS 13, PASS1_BITS 2 ------------------------------------------------------------------------------
// One 1-D pass over eight values: out = DESCALE(..., shift), an arithmetic shift.
CDN_JPEG_HD void idct_1d(const int (&in)[8], int (&out)[8], int shift) {
  typedef uint32_t u;
  const u half = (u)1 << (shift - 1);
  const u i0 = (u)in[0], i1 = (u)in[1], i2 = (u)in[2], i3 = (u)in[3], i4 = (u)in[4], i5 = (u)in[5], i6 = (u)in[6],
          i7 = (u)in[7];
  u z1 = (i2 + i6) * 4433u;
  const u e2 = z1 - i6 * 15137u;
  const u e3 = z1 + i2 * 6270u;
  const u e0 = (i0 + i4) << 13;
  const u e1 = (i0 - i4) << 13;
  const u t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  u t0 = i7, t1 = i5, t2 = i3, t3 = i1;
  z1 = t0 + t3;
  u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const u z5 = (z3 + z4) * 9633u;
  t0 *= 2446u;
  t1 *= 16819u;
  t2 *= 25172u;
  t3 *= 12299u;
  z1 = (u)0 - z1 * 7373u;
  z2 = (u)0 - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  out[0] = (int32_t)(t10 + t3 + half) >> shift;
  out[7] = (int32_t)(t10 - t3 + half) >> shift;
  out[1] = (int32_t)(t11 + t2 + half) >> shift;
  out[6] = (int32_t)(t11 - t2 + half) >> shift;
  out[2] = (int32_t)(t12 + t1 + half) >> shift;
  out[5] = (int32_t)(t12 - t1 + half) >> shift;
  out[3] = (int32_t)(t13 + t0 + half) >> shift;
  out[4] = (int32_t)(t13 - t0 + half) >> shift;
}
CDN_JPEG_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// pass 1: column c of a block, tile -> ws
CDN_JPEG_HD void idct_column(const int *tile, int *ws, int c) {
  int in[8], out[8];
  for (int r = 0; r < 8; ++r) in[r] = tile[r * 8 + c];
  idct_1d(in, out, 11);
  for (int r = 0; r < 8; ++r) ws[r * 8 + c] = out[r];
}
// pass 2: row r of a block, ws -> eight samples as one 64-bit word (sample x in byte x)
CDN_JPEG_HD uint64_t idct_row(const int *ws, int r) {
  int in[8], out[8];
  for (int x = 0; x < 8; ++x) in[x] = ws[r * 8 + x];
  idct_1d(in, out, 18);
  uint64_t v = 0;
  for (int x = 0; x < 8; ++x) v |= (uint64_t)clamp255(out[x] + 128) << (8 * x);
  return v;
}
// (planes and pitches are multiples of 8 bytes; little-endian on both sides)
CDN_JPEG_HD void store8(uint8_t *p, uint64_t v) { *reinterpret_cast<uint64_t *>(p) = v; }

// where block b of MCU (mx, my) lives: its component and the plane address of its first sample
CDN_JPEG_HD uint8_t *block_origin(const Geom &g, uint8_t *planes, int mx, int my, int b, int *comp, int *pitch) {
  const int ny = g.hs * g.vs;
  if (b < ny) {
    const int bx = b % g.hs, by = b / g.hs;
    *comp = 0;
    *pitch = g.pitch_y;
    return planes + (int64_t)((my * g.vs + by) * 8) * g.pitch_y + (mx * g.hs + bx) * 8;
  }
  *comp = 1 + (b - ny);
  *pitch = g.pitch_c;
  return planes + (int64_t)g.pitch_y * g.rows_y + (int64_t)(b - ny) * g.pitch_c * g.rows_c +
         (int64_t)(my * 8) * g.pitch_c + mx * 8;
}

struct NoSync {
  CDN_JPEG_HD void operator()() const {}
};

constexpr int kWindow = 2048;       // bytes of the stream window
constexpr int kWindowLow = 1024;    // refilled in front of an MCU that starts with fewer bytes than this left in it

// One segment.  `lane` of `nlanes` callers run this together (the kernel: the 64 lanes of a wave; the host: one);
// sync() orders their accesses to tile / ws / win / flag (a barrier; nothing on the host).  Lane 0 decodes the MCU's
// blocks, every lane takes columns and rows of the two IDCT passes (eight per block) and a share of the window refill.
// tile, ws: 6 * 64 ints each, tile ZEROED on entry and on return; win: kWindow bytes, through which the segment's bytes
// reach the bit reader (all lanes copy the next 2 KB between two MCUs; without it every refill of lane 0's bit reader is
// a round trip to global memory in the middle of the chain; an MCU that runs past the window reads the rest from p);
// flag: two ints.  -> the segment's status, the same in every lane.
template <class Sync>
CDN_JPEG_HD int decode_segment(const Segment &sg, const Tables *tab, uint8_t *item_planes, int *tile, int *ws, uint8_t *win,
                               int *flag, int lane, int nlanes, Sync sync) {
  const Geom &g = sg.g;
  const int nblk = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;          // <= 6
  Bits br;
  bits_init(&br, sg.bytes, sg.len);
  int pred[3] = {0, 0, 0};
  br.win = win;
  int status = 0, pos = 0, wbase = 0, wend = 0;       // pos: where lane 0's reader stands; the same in every lane
  for (int m = 0; m < sg.count; ++m) {
    const int mi = sg.first + m, my = mi / g.mcus_x, mx = mi - my * g.mcus_x;
    if (wend < sg.len && pos + kWindowLow > wend) {    // (nobody reads win between the last barrier of an MCU and here)
      wbase = pos;
      const int n = sg.len - wbase < kWindow ? sg.len - wbase : kWindow;
      for (int i = lane; i < n; i += nlanes) win[i] = sg.bytes[wbase + i];
      wend = wbase + n;
      sync();
    }
    if (lane == 0) {
      br.wbase = wbase;
      br.wend = wend;
      int err = 0;
      for (int b = 0; b < nblk && !err; ++b) {
        const int comp = g.ncomp == 1 ? 0 : (b < nblk - 2 ? 0 : b - (nblk - 2) + 1);
        const Huff *dc = &tab->huff[(g.sel >> (2 * comp)) & 1], *ac = &tab->huff[2 + ((g.sel >> (2 * comp + 1)) & 1)];
        err = decode_block(&br, dc, ac, tab->quant[comp], tab->zigzag, &pred[comp], tile + b * 64);
      }
      if (!err && br.real < 0) err = kOverread;
      flag[0] = err;
      flag[1] = br.pos;
    }
    sync();
    status = flag[0];
    pos = flag[1];
    for (int t = lane; t < nblk * 8; t += nlanes) idct_column(tile + (t >> 3) * 64, ws + (t >> 3) * 64, t & 7);
    sync();
    for (int t = lane; t < nblk * 8; t += nlanes) {
      const int b = t >> 3, r = t & 7;
      int comp, pitch;
      uint8_t *o = block_origin(g, item_planes, mx, my, b, &comp, &pitch);
      store8(o + (int64_t)r * pitch, idct_row(ws + b * 64, r));
      for (int x = 0; x < 8; ++x) tile[b * 64 + r * 8 + x] = 0;
    }
    sync();
    if (status) break;        // (uniform: every lane read the same flag)
  }
  return status;
}

// ---- fancy up-sampling and colour: output pixels 2i and 2i + 1 of row y ---------------------------------------------------
CDN_JPEG_HD void store_pixel(uint8_t *o, int yy, int cb, int cr, int rgb) {
  cb -= 128;
  cr -= 128;
  const int R = clamp255(yy + ((91881 * cr + 32768) >> 16));
  const int B = clamp255(yy + ((116130 * cb + 32768) >> 16));
  const int G = clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  o[0] = (uint8_t)(rgb ? R : B);
  o[1] = (uint8_t)G;
  o[2] = (uint8_t)(rgb ? B : R);
}
CDN_JPEG_HD void color_pair(const Geom &g, const uint8_t *planes, uint8_t *out, int y, int i, int rgb) {
  const int x0 = 2 * i;
  const bool two = x0 + 1 < g.w;
  const uint8_t *py = planes + (int64_t)y * g.pitch_y + x0;
  uint8_t *o = out + g.out_off + (int64_t)y * g.out_pitch + 3 * (int64_t)x0;
  const int y0 = py[0], y1 = two ? py[1] : 0;
  if (g.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)y0;
    if (two) o[3] = o[4] = o[5] = (uint8_t)y1;
    return;
  }
  const uint8_t *pcb = planes + (int64_t)g.pitch_y * g.rows_y, *pcr = pcb + (int64_t)g.pitch_c * g.rows_c;
  int c0[2], c1[2];       // [cb, cr] of the two pixels
  if (g.mode == 0) {
    const int64_t a = (int64_t)y * g.pitch_c + x0;
    c0[0] = pcb[a];
    c0[1] = pcr[a];
    c1[0] = two ? pcb[a + 1] : 0;
    c1[1] = two ? pcr[a + 1] : 0;
  } else {
    const int n = (g.w + 1) / 2;                                  // true chroma width
    const int il = i > 0 ? i - 1 : 0, ir = i + 1 < n ? i + 1 : n - 1;
    if (g.mode == 1) {
      const int64_t row = (int64_t)y * g.pitch_c;
      for (int c = 0; c < 2; ++c) {
        const uint8_t *p = (c ? pcr : pcb) + row;
        const int v = p[i];
        c0[c] = i == 0 ? v : (3 * v + p[il] + 1) >> 2;
        c1[c] = i == n - 1 ? v : (3 * v + p[ir] + 2) >> 2;
      }
    } else {
      const int nr = (g.h + 1) / 2;                               // true chroma height
      const int r = y >> 1;
      int rn = (y & 1) ? r + 1 : r - 1;
      rn = rn < 0 ? 0 : (rn > nr - 1 ? nr - 1 : rn);
      for (int c = 0; c < 2; ++c) {
        const uint8_t *p = (c ? pcr : pcb) + (int64_t)r * g.pitch_c, *q = (c ? pcr : pcb) + (int64_t)rn * g.pitch_c;
        const int s = 3 * p[i] + q[i], sl = 3 * p[il] + q[il], sr = 3 * p[ir] + q[ir];
        c0[c] = i == 0 ? (4 * s + 8) >> 4 : (3 * s + sl + 8) >> 4;
        c1[c] = i == n - 1 ? (4 * s + 7) >> 4 : (3 * s + sr + 7) >> 4;
      }
    }
  }
  store_pixel(o, y0, c0[0], c0[1], rgb);
  if (two) store_pixel(o + 3, y1, c1[0], c1[1], rgb);
}

// planes -> interleaved pixels of every item, on one thread
inline void color_host(const Call &c) {
  const int ni = n_items(c);
  for (int item = 0; item < ni; ++item) {
    Geom g;
    if (!item_geom(c.items + (int64_t)item * kItemWords, c.plane_stride, &g) || !out_fits(g, c.out_cap)) {
      if (c.status[item] < kBadRecord) c.status[item] = kBadRecord;
      continue;
    }
    const uint8_t *planes = c.planes + item * c.plane_stride;
    const int pw = (g.w + 1) / 2;
    for (int y = 0; y < g.h; ++y)
      for (int i = 0; i < pw; ++i) color_pair(g, planes, c.out, y, i, c.rgb);
  }
}

// ---- the whole call on one thread: what cdn_jpeg_decode_host runs ---------------------------------------------------------
inline void decode_host(const Call &c) {
  int tile[6 * 64], ws[6 * 64], flag[2] = {0, 0};
  uint8_t win[kWindow];
  memset(tile, 0, sizeof(tile));
  const int ns = n_segments(c), ni = n_items(c);
  for (int s = 0; s < ns; ++s) {
    Segment sg;
    if (!segment_geom(c, s, &sg)) {
      const int item = c.segs[(int64_t)(1 + s) * kSegWords + kSegItem];
      if (item >= 0 && item < ni && c.status[item] < kBadRecord) c.status[item] = kBadRecord;
      continue;
    }
    const Tables *tab = reinterpret_cast<const Tables *>(c.tables + (int64_t)sg.item * kTableBytes);
    const int st = decode_segment(sg, tab, c.planes + sg.item * c.plane_stride, tile, ws, win, flag, 0, 1, NoSync());
    if (st > c.status[sg.item]) c.status[sg.item] = st;
  }
  color_host(c);
}

// ==== the parallel entropy path: one segment on the lanes of a workgroup ==================================================
// The host removed the byte stuffing, so a segment is a plain bit string: it is cut into sub-sequences of S bits, W of
// them form a tile, and lane j of the workgroup decodes sub-sequence j of the tile.  The decoder state at a bit position is
// (p, b, z): p the position, b the block within the MCU (it selects the tables), z the zig-zag position (0: a DC symbol
// is next); DC prediction is NOT part of it, the entropy pass stores DC differences.  A state can also be dead: a bad code
// was met or the bits ran out.  Per tile: a dry pass from a cold state (p = start of the sub-sequence, 0, 0; lane 0 has
// the exact state the tile before it left), counted rounds in which lane j decodes again from the exit of lane j - 1
// whenever that differs from the entry it used last (after round r lanes 0..r are exact by induction, so W - 1 rounds
// always suffice; Huffman streams self-synchronise, so two or three usually do), an exclusive prefix sum of the blocks
// each lane completed, and a write pass that stores raw coefficients (int16, natural order, at block * 64 + n) and DC
// differences (a word per block) into the item's workspace.  After the last tile the DC differences become predictions
// (an inclusive scan per component) and the status follows from the exact chain alone.  Every loop is counted: a symbol
// consumes at least one bit, so a sub-sequence decode runs at most S times, and a block index at or beyond count * nblk
// stores nothing -- that is the bounds check.
constexpr int kParLanes = 256;                        // W: lanes of the workgroup = sub-sequences of a tile
constexpr int kParWindow = kParLanes * 128 + 64;      // bytes of a tile of 1024-bit sub-sequences, and its look-ahead
constexpr int kParMaxLen = (1 << 28) - (1 << 19);     // 8 len + W S + 64 stays below 2^31: bit positions are ints
static_assert(kParLanes == 256, "par_scan: an even number of doubling steps leaves the sums in place");

CDN_JPEG_HD bool subseq_bits_ok(int s) { return s >= 64 && s <= 8192 && s % 32 == 0; }
// per item: blocks the planes can hold, their coefficients (64 int16) and DC words
CDN_JPEG_HD int64_t par_blocks(int64_t plane_stride_) { return plane_stride_ / 64; }
CDN_JPEG_HD int64_t par_work_stride(int64_t plane_stride_) { return (par_blocks(plane_stride_) * 132 + 15) / 16 * 16; }

struct alignas(16) Coef8 {          // one row of a block's coefficients
  int16_t v[8];
};
struct ParCall {
  Call c;
  uint8_t *work;                    // per item: int16 coef[blocks][64], then int32 dc[blocks]
  int64_t work_stride;
  int subseq_bits;
};
CDN_JPEG_HD int16_t *par_coef(const ParCall &pc, int item) {
  return reinterpret_cast<int16_t *>(pc.work + (int64_t)item * pc.work_stride);
}
CDN_JPEG_HD int32_t *par_dc(const ParCall &pc, int item) {
  return reinterpret_cast<int32_t *>(pc.work + (int64_t)item * pc.work_stride + par_blocks(pc.c.plane_stride) * 128);
}

typedef uint64_t PState;            // p << 32 | why << 16 | b << 8 | z; why != 0: dead, and nothing else is set
CDN_JPEG_HD PState ps_make(int p, int b, int z) { return ((uint64_t)(uint32_t)p << 32) | ((uint32_t)b << 8) | (uint32_t)z; }
CDN_JPEG_HD PState ps_dead(int why) { return (uint64_t)why << 16; }
CDN_JPEG_HD int ps_why(PState s) { return (int)(s >> 16) & 3; }

// 32 more bits at any byte position: zeros beyond the segment, and pos always moves on, so the bit position of the next
// unread bit is 8 pos - n
CDN_JPEG_HD void par_fill(Bits *b) {
  if (b->n > 32) return;
  uint32_t v = 0;
  const int pos = b->pos;
  if (pos >= b->wbase && pos + 4 <= b->wend) {      // (the window holds zeros beyond the segment)
    v = load_be32(b->win + (pos - b->wbase));
  } else if (pos + 4 <= b->len) {
    v = load_be32(b->p + pos);
  } else {
    for (int i = 0; i < 4; ++i)
      if (pos + i < b->len) v |= (uint32_t)b->p[pos + i] << (24 - 8 * i);
  }
  b->pos = pos + 4;
  b->acc |= (uint64_t)v << (32 - b->n);
  b->n += 32;
}

// what a sub-sequence decode needs beside its entry state
struct ParSeg {
  Bits src;                         // bytes, length and window of the segment
  const Tables *tab;
  int sel, ncomp, nblk;
  int total_bits;                   // 8 len
  int limit;                        // count * nblk: blocks of the segment
  int16_t *coef;                    // of the segment's first block
  int32_t *dc;
};

// The symbols that START in [p of entry, end).  -> the exit state: that of the first symbol start at or beyond `end`, or
// dead; *done = blocks completed (EOB or k reaching 64).  An entry at or beyond `end`, or a dead one, is its own exit.
// kStore: coefficients and DC differences of blocks below the limit are stored, `blk` being the block the entry lies in.
template <bool kStore>
CDN_JPEG_HD PState par_subseq(const ParSeg &ps, PState entry, int end, int blk, int *done) {
  *done = 0;
  if (ps_why(entry)) return entry;
  int p = (int)(entry >> 32), b = (int)(entry >> 8) & 7, z = (int)entry & 127;
  if (p >= end) return entry;
  Bits br = ps.src;
  br.pos = p >> 3;
  br.acc = 0;
  br.n = 0;
  br.real = 0;
  par_fill(&br);
  bits_skip(&br, p & 7);
  int n = 0;
  while (p < end) {                 // p grows by at least 1 per iteration
    if (kStore && blk >= ps.limit) break;
    par_fill(&br);
    const int comp = ps.ncomp == 1 ? 0 : (b < ps.nblk - 2 ? 0 : b - (ps.nblk - 2) + 1);
    const Huff *t = &ps.tab->huff[z == 0 ? (ps.sel >> (2 * comp)) & 1 : 2 + ((ps.sel >> (2 * comp + 1)) & 1)];
    const int sym = huff_symbol(&br, t);
    if (sym < 0) {                  // with real bits in all 16 places it is a bad code; otherwise the bits ran out
      *done = n;
      return ps_dead(p + 16 > ps.total_bits ? kOverread : kBadCode);
    }
    const int tb = sym & 15;
    const int v = tb ? receive_extend(&br, tb) : 0;        // (<= 16 + 15 bits since the fill)
    const int q = 8 * br.pos - br.n;                       // where the next symbol starts
    if (q > ps.total_bits) {        // the symbol needed bits beyond the end
      *done = n;
      return ps_dead(kOverread);
    }
    p = q;
    if (z == 0) {
      if (kStore) ps.dc[blk] = v;
      z = 1;
    } else if (tb) {
      z += sym >> 4;
      if (kStore && z < 64) ps.coef[(int64_t)blk * 64 + (ps.tab->zigzag[z] & 63)] = (int16_t)v;
      z += 1;
    } else if ((sym >> 4) == 15) {
      z += 16;                      // ZRL
    } else {
      z = 64;                       // EOB
    }
    if (z >= 64) {
      ++n;
      ++blk;
      b = b + 1 == ps.nblk ? 0 : b + 1;
      z = 0;
    }
  }
  *done = n;
  return ps_make(p, b, z);
}

// inclusive sums (uint32 wrap-around) of a[0 .. W) in place; tmp: W more words.  The caller's last sync() is behind the
// writes of a.
template <class Sync>
CDN_JPEG_HD void par_scan(uint32_t *a, uint32_t *tmp, int lane, int nlanes, Sync sync) {
  uint32_t *src = a, *dst = tmp;
  for (int d = 1; d < kParLanes; d <<= 1) {
    for (int j = lane; j < kParLanes; j += nlanes) dst[j] = src[j] + (j >= d ? src[j - d] : 0u);
    sync();
    uint32_t *t = src;
    src = dst;
    dst = t;
  }
}

// the workgroup's shared arrays (LDS on the device)
struct ParShared {
  PState *exit;                     // [2][W]: the exits of the round before and of this round
  PState *entry;                    // [W]: the entry each lane used last
  int *cnt;                         // [W]: blocks each lane completed
  uint32_t *scan;                   // [4][W]
  int *flag;                        // [3]: "an exit changed" of rounds r % 3
  uint8_t *win;                     // [kParWindow]: the tile's bytes
};

// One segment.  `lane` of `nlanes` callers run this together (the kernel: the W lanes of a workgroup; the host: one, which
// takes every j in turn); sync() is a barrier that every caller reaches the same number of times -- the conditions around
// it depend on the segment record and on words all callers read behind a sync() alone.  -> the status, the same in every
// caller.
template <class Sync>
CDN_JPEG_HD int decode_segment_parallel(const Segment &sg, const Tables *tab, int16_t *item_coef, int32_t *item_dc, int S,
                                        const ParShared &sh, int lane, int nlanes, Sync sync) {
  constexpr int W = kParLanes;
  const Geom &g = sg.g;
  if (sg.len > kParMaxLen) return kBadRecord;
  ParSeg ps;
  bits_init(&ps.src, sg.bytes, sg.len);
  ps.src.win = sh.win;
  ps.tab = tab;
  ps.sel = g.sel;
  ps.ncomp = g.ncomp;
  ps.nblk = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;          // <= 6
  ps.total_bits = 8 * sg.len;
  ps.limit = sg.count * ps.nblk;
  ps.coef = item_coef + (int64_t)sg.first * ps.nblk * 64;
  ps.dc = item_dc + (int64_t)sg.first * ps.nblk;
  // the segment's blocks start as zeros: what the image needs, not the capacity (a block is 8 rows of 16 bytes, and the
  // workspace is 16-byte aligned)
  Coef8 *clear = reinterpret_cast<Coef8 *>(ps.coef);
  for (int64_t i = lane; i < (int64_t)ps.limit * 8; i += nlanes) clear[i] = Coef8{{0, 0, 0, 0, 0, 0, 0, 0}};
  for (int i = lane; i < ps.limit; i += nlanes) ps.dc[i] = 0;
  sync();
  const int nsub = (ps.total_bits + S - 1) / S, ntiles = (nsub + W - 1) / W;
  PState carry = ps_make(0, 0, 0);
  int carry_blk = 0;
  for (int t = 0; t < ntiles; ++t) {
    const int sub0 = t * W;
    // the tile's bytes and 64 of look-ahead, zeros beyond the segment
    const int wbase = sub0 * (S / 8), avail = sg.len - wbase, tile_bytes = W * (S / 8);
    int wn = (avail < tile_bytes ? avail : tile_bytes) + 64;
    wn = wn < kParWindow ? wn : kParWindow;
    for (int i = lane; i < wn; i += nlanes) sh.win[i] = wbase + i < sg.len ? sg.bytes[wbase + i] : (uint8_t)0;
    if (lane == 0) sh.flag[1] = 0;
    sync();
    ps.src.wbase = wbase;
    ps.src.wend = wbase + wn;
    // dry pass: lane 0 from the exact state, every other lane cold; na: the sub-sequences of this tile -- the lanes that
    // take part (a lane beyond them completes no block)
    const int na = nsub - sub0 < W ? nsub - sub0 : W;
    for (int j = lane; j < W; j += nlanes) {
      const int start = (sub0 + j) * S;
      int n = 0;
      if (j < na) {
        sh.entry[j] = j == 0 ? carry : ps_make(start, 0, 0);
        sh.exit[j] = par_subseq<false>(ps, sh.entry[j], start + S, 0, &n);
      }
      sh.cnt[j] = n;
    }
    sync();
    // synchronisation rounds: after round r the lanes 0 .. r are exact, so na - 1 rounds always suffice
    int cur = 0;
    for (int r = 1; r < na; ++r) {
      const PState *prev = sh.exit + cur * W;
      cur ^= 1;
      PState *next = sh.exit + cur * W;
      for (int j = lane; j < na; j += nlanes) {
        PState x = prev[j];
        if (j > 0 && prev[j - 1] != sh.entry[j]) {
          int n;
          sh.entry[j] = prev[j - 1];
          const PState y = par_subseq<false>(ps, sh.entry[j], (sub0 + j + 1) * S, 0, &n);
          sh.cnt[j] = n;
          if (y != x) sh.flag[r % 3] = 1;
          x = y;
        }
        next[j] = x;
      }
      if (lane == 0) sh.flag[(r + 1) % 3] = 0;
      sync();
      if (!sh.flag[r % 3]) break;   // (uniform: every caller reads the word behind the same sync)
    }
    // block indices: exclusive prefix sum of the counts
    for (int j = lane; j < W; j += nlanes) sh.scan[j] = (uint32_t)sh.cnt[j];
    sync();
    par_scan(sh.scan, sh.scan + W, lane, nlanes, sync);
    // write pass
    for (int j = lane; j < na; j += nlanes) {
      int n;
      par_subseq<true>(ps, sh.entry[j], (sub0 + j + 1) * S, carry_blk + (int)sh.scan[j] - sh.cnt[j], &n);
    }
    carry = sh.exit[cur * W + na - 1];
    carry_blk += (int)sh.scan[W - 1];
    sync();
  }
  // DC differences -> predictions: lane j takes MCUs [j per, (j + 1) per)
  const int per = (sg.count + W - 1) / W;
  for (int j = lane; j < W; j += nlanes) {
    uint32_t sum[3] = {0, 0, 0};
    for (int m = j * per; m < (j + 1) * per && m < sg.count; ++m)
      for (int b = 0; b < ps.nblk; ++b)
        sum[ps.ncomp == 1 || b < ps.nblk - 2 ? 0 : b - (ps.nblk - 2) + 1] += (uint32_t)ps.dc[m * ps.nblk + b];
    for (int c = 0; c < 3; ++c) sh.scan[c * W + j] = sum[c];
  }
  sync();
  for (int c = 0; c < ps.ncomp; ++c) par_scan(sh.scan + c * W, sh.scan + 3 * W, lane, nlanes, sync);
  for (int j = lane; j < W; j += nlanes) {
    uint32_t pred[3];
    for (int c = 0; c < 3; ++c) pred[c] = j > 0 ? sh.scan[c * W + j - 1] : 0u;
    for (int m = j * per; m < (j + 1) * per && m < sg.count; ++m)
      for (int b = 0; b < ps.nblk; ++b) {
        const int c = ps.ncomp == 1 || b < ps.nblk - 2 ? 0 : b - (ps.nblk - 2) + 1;
        pred[c] += (uint32_t)ps.dc[m * ps.nblk + b];
        ps.dc[m * ps.nblk + b] = (int32_t)pred[c];
      }
  }
  sync();
  // the exact chain alone decides: complete, or why it stopped short
  return carry_blk >= ps.limit ? 0 : (ps_why(carry) == kBadCode ? kBadCode : kOverread);
}

// block `blk` of an item (MCU-interleaved order): coefficient row r, dequantised, into tile[r * 8 ..]
CDN_JPEG_HD void par_dequant_row(const int16_t *coef, const int32_t *dc, int64_t blk, const uint8_t *q, int r, int *tile) {
  const Coef8 c8 = *reinterpret_cast<const Coef8 *>(coef + blk * 64 + r * 8);
  for (int x = 0; x < 8; ++x) tile[r * 8 + x] = (int)((uint32_t)(int)c8.v[x] * (uint32_t)q[r * 8 + x]);
  if (r == 0) tile[0] = (int)((uint32_t)dc[blk] * (uint32_t)q[0]);
}
CDN_JPEG_HD int block_comp(const Geom &g, int b) {
  const int ny = g.hs * g.vs;
  return g.ncomp == 1 || b < ny ? 0 : 1 + (b - ny);
}

// ---- the whole parallel call on one thread: what cdn_jpeg_decode_parallel_host runs ---------------------------------------
inline void decode_host_parallel(const ParCall &pc) {
  const Call &c = pc.c;
  PState exit_[2 * kParLanes], entry[kParLanes];
  int cnt[kParLanes], flag[3] = {0, 0, 0};
  uint32_t scan[4 * kParLanes];
  uint8_t win[kParWindow];
  const ParShared sh{exit_, entry, cnt, scan, flag, win};
  const int ns = n_segments(c), ni = n_items(c);
  for (int s = 0; s < ns; ++s) {
    Segment sg;
    if (!segment_geom(c, s, &sg)) {
      const int item = c.segs[(int64_t)(1 + s) * kSegWords + kSegItem];
      if (item >= 0 && item < ni && c.status[item] < kBadRecord) c.status[item] = kBadRecord;
      continue;
    }
    const Tables *tab = reinterpret_cast<const Tables *>(c.tables + (int64_t)sg.item * kTableBytes);
    const int st = decode_segment_parallel(sg, tab, par_coef(pc, sg.item), par_dc(pc, sg.item), pc.subseq_bits, sh, 0, 1,
                                           NoSync());
    if (st > c.status[sg.item]) c.status[sg.item] = st;
  }
  for (int item = 0; item < ni; ++item) {
    Geom g;
    if (!item_geom(c.items + (int64_t)item * kItemWords, c.plane_stride, &g)) continue;      // (color_host sets the status)
    const Tables *tab = reinterpret_cast<const Tables *>(c.tables + (int64_t)item * kTableBytes);
    const int nblk = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    const int64_t total = (int64_t)g.mcus_x * g.mcus_y * nblk;
    int tile[64], ws[64];
    for (int64_t blk = 0; blk < total; ++blk) {
      const int mi = (int)(blk / nblk), b = (int)(blk - (int64_t)mi * nblk), my = mi / g.mcus_x, mx = mi - my * g.mcus_x;
      int comp, pitch;
      uint8_t *o = block_origin(g, c.planes + item * c.plane_stride, mx, my, b, &comp, &pitch);
      for (int r = 0; r < 8; ++r) par_dequant_row(par_coef(pc, item), par_dc(pc, item), blk, tab->quant[comp], r, tile);
      for (int col = 0; col < 8; ++col) idct_column(tile, ws, col);
      for (int r = 0; r < 8; ++r) store8(o + (int64_t)r * pitch, idct_row(ws, r));
    }
  }
  color_host(c);
}

// ==== host half: header parse, decode tables, byte packing ================================================================
enum ParseResult { kParsed = 0, kMalformed = -1, kUnsupported = -5 };      // (the values of CDN_ERR_ARG / CDN_ERR_UNSUPPORTED)

struct Header {
  int w, h, ncomp, mode, mcus_x, mcus_y, restart, n_segments;
  int tq[3], td[3], ta[3];
  int64_t scan_off;                 // first byte of the entropy-coded data
  uint8_t quant[4][64];             // natural order
  uint8_t bits[4][17];              // [DC 0, DC 1, AC 0, AC 1][length]
  uint8_t vals[4][256];
  bool have_q[4], have_h[4];
};

#define CDN_JPEG_FAIL(code, ...)               \
  do {                                         \
    snprintf(msg, msg_len, __VA_ARGS__);       \
    return code;                               \
  } while (0)

inline int total_mcus(const Header &hd) { return hd.mcus_x * hd.mcus_y; }
inline int expected_segments(const Header &hd) {
  return hd.restart > 0 ? (total_mcus(hd) + hd.restart - 1) / hd.restart : 1;
}

// Walk the entropy-coded bytes from scan_off.  sink(kind, p, n): kind 0 = n plain bytes at p, 1 = one 0xFF (its stuffed 00
// removed), 2 = a restart marker (the segment ends).  -> kParsed at EOI or at the end of the data.
template <class Sink>
inline int walk_scan(const uint8_t *d, int64_t n, int64_t pos, Sink &sink, char *msg, size_t msg_len) {
  while (pos < n) {
    const uint8_t *ff = static_cast<const uint8_t *>(memchr(d + pos, 0xFF, (size_t)(n - pos)));
    const int64_t run = ff ? ff - (d + pos) : n - pos;
    if (run) {
      const int rc = sink(0, d + pos, run);
      if (rc) return rc;
      pos += run;
    }
    if (!ff) break;
    int64_t q = pos + 1;
    while (q < n && d[q] == 0xFF) ++q;          // fill bytes in front of a marker
    if (q >= n) break;                          // the data ends inside a marker: as a missing EOI
    const int m = d[q];
    pos = q + 1;
    if (m == 0x00) {
      const int rc = sink(1, nullptr, 1);
      if (rc) return rc;
    } else if (m >= 0xD0 && m <= 0xD7) {
      const int rc = sink(2, nullptr, 0);
      if (rc) return rc;
    } else if (m == 0xD9) {
      return kParsed;
    } else if (m == 0xDC) {
      CDN_JPEG_FAIL(kUnsupported, "DNL marker: not supported");
    } else {
      CDN_JPEG_FAIL(kUnsupported, "marker 0x%02X inside the scan: several scans are not supported", m);
    }
  }
  return kParsed;
}

inline int parse(const uint8_t *d, int64_t n, Header *hd, char *msg, size_t msg_len) {
  memset(hd, 0, sizeof(*hd));
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) CDN_JPEG_FAIL(kMalformed, "not a JPEG stream (no SOI)");
  int64_t pos = 2;
  bool have_sof = false, adobe_rgb = false;
  int comp_id[3] = {0, 0, 0}, hv[3] = {0, 0, 0};
  for (;;) {
    if (pos >= n) CDN_JPEG_FAIL(kMalformed, "the data ends before the scan");
    if (d[pos] != 0xFF) CDN_JPEG_FAIL(kMalformed, "byte 0x%02X at %lld where a marker must be", d[pos], (long long)pos);
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) CDN_JPEG_FAIL(kMalformed, "the data ends before the scan");
    const int m = d[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD8 || m == 0xD9 || m == 0x00) CDN_JPEG_FAIL(kMalformed, "marker 0x%02X in the header", m);
    if (pos + 2 > n) CDN_JPEG_FAIL(kMalformed, "truncated marker segment");
    const int64_t len = (d[pos] << 8) | d[pos + 1];
    if (len < 2 || pos + len > n) CDN_JPEG_FAIL(kMalformed, "marker 0x%02X: length %lld beyond the data", m, (long long)len);
    const uint8_t *p = d + pos + 2;
    const int64_t body = len - 2;
    pos += len;
    if (m == 0xC0) {
      if (have_sof) CDN_JPEG_FAIL(kMalformed, "two frame headers");
      if (body < 6) CDN_JPEG_FAIL(kMalformed, "short SOF0");
      if (p[0] != 8) CDN_JPEG_FAIL(kUnsupported, "%d-bit samples: not supported", p[0]);
      hd->h = (p[1] << 8) | p[2];
      hd->w = (p[3] << 8) | p[4];
      hd->ncomp = p[5];
      if (hd->h == 0) CDN_JPEG_FAIL(kUnsupported, "height 0 (DNL): not supported");
      if (hd->w == 0) CDN_JPEG_FAIL(kMalformed, "width 0");
      if (hd->ncomp != 1 && hd->ncomp != 3) CDN_JPEG_FAIL(kUnsupported, "%d components: not supported", hd->ncomp);
      if (body != 6 + 3 * hd->ncomp) CDN_JPEG_FAIL(kMalformed, "SOF0 length");
      for (int c = 0; c < hd->ncomp; ++c) {
        comp_id[c] = p[6 + 3 * c];
        hv[c] = p[7 + 3 * c];
        hd->tq[c] = p[8 + 3 * c];
        if (hd->tq[c] > 3) CDN_JPEG_FAIL(kMalformed, "quantisation table selector %d", hd->tq[c]);
        if ((hv[c] >> 4) < 1 || (hv[c] >> 4) > 4 || (hv[c] & 15) < 1 || (hv[c] & 15) > 4)
          CDN_JPEG_FAIL(kMalformed, "sampling factors 0x%02X", hv[c]);
      }
      have_sof = true;
    } else if (m == 0xC4) {
      int64_t o = 0;
      while (o < body) {
        if (o + 17 > body) CDN_JPEG_FAIL(kMalformed, "short DHT");
        const int tc = p[o] >> 4, th = p[o] & 15;
        if (tc > 1 || th > 3) CDN_JPEG_FAIL(kMalformed, "Huffman table class %d id %d", tc, th);
        if (th > 1) CDN_JPEG_FAIL(kUnsupported, "Huffman table id %d: baseline has 0 and 1", th);
        const int t = tc * 2 + th;
        int count = 0;
        hd->bits[t][0] = 0;
        for (int l = 1; l <= 16; ++l) count += (hd->bits[t][l] = p[o + l]);
        if (count > 256 || o + 17 + count > body) CDN_JPEG_FAIL(kMalformed, "DHT with %d symbols", count);
        memset(hd->vals[t], 0, 256);
        memcpy(hd->vals[t], p + o + 17, (size_t)count);
        hd->have_h[t] = true;
        o += 17 + count;
      }
    } else if (m == 0xDB) {
      int64_t o = 0;
      while (o < body) {
        const int pq = p[o] >> 4, tq = p[o] & 15;
        if (pq > 1 || tq > 3) CDN_JPEG_FAIL(kMalformed, "quantisation table precision %d id %d", pq, tq);
        if (pq == 1) CDN_JPEG_FAIL(kUnsupported, "16-bit quantisation table: not supported");
        if (o + 65 > body) CDN_JPEG_FAIL(kMalformed, "short DQT");
        for (int k = 0; k < 64; ++k) hd->quant[tq][zigzag(k)] = p[o + 1 + k];
        hd->have_q[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {
      if (body != 2) CDN_JPEG_FAIL(kMalformed, "DRI length");
      hd->restart = (p[0] << 8) | p[1];
    } else if (m == 0xEE) {
      if (body >= 12 && memcmp(p, "Adobe", 5) == 0 && p[11] == 0) adobe_rgb = true;
    } else if (m == 0xDA) {
      if (!have_sof) CDN_JPEG_FAIL(kMalformed, "scan before the frame header");
      if (body < 1) CDN_JPEG_FAIL(kMalformed, "short SOS");
      const int ns = p[0];
      if (ns < 1 || ns > 4 || body != 4 + 2 * ns) CDN_JPEG_FAIL(kMalformed, "SOS length");
      if (ns != hd->ncomp) CDN_JPEG_FAIL(kUnsupported, "a scan of %d of %d components: several scans are not supported", ns,
                                         hd->ncomp);
      for (int c = 0; c < ns; ++c) {
        if (p[1 + 2 * c] != comp_id[c]) CDN_JPEG_FAIL(kUnsupported, "scan components out of frame order: not supported");
        hd->td[c] = p[2 + 2 * c] >> 4;
        hd->ta[c] = p[2 + 2 * c] & 15;
        if (hd->td[c] > 1 || hd->ta[c] > 1) CDN_JPEG_FAIL(kUnsupported, "Huffman table selector beyond 1");
        if (!hd->have_h[hd->td[c]] || !hd->have_h[2 + hd->ta[c]]) CDN_JPEG_FAIL(kMalformed, "scan names a missing Huffman table");
        if (!hd->have_q[hd->tq[c]]) CDN_JPEG_FAIL(kMalformed, "frame names a missing quantisation table");
      }
      if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0)
        CDN_JPEG_FAIL(kUnsupported, "spectral selection / successive approximation: not supported");
      hd->scan_off = pos;
      break;
    } else if (m == 0xC2 || m == 0xC1 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8)) {
      CDN_JPEG_FAIL(kUnsupported, "frame type 0x%02X (progressive, extended, lossless or arithmetic): only SOF0 is supported", m);
    }      // every other segment (APPn, COM, ...) is skipped; EXIF orientation is ignored
  }
  // sampling
  if (hd->ncomp == 1) {
    if (hv[0] != 0x11) CDN_JPEG_FAIL(kUnsupported, "grey stream with sampling 0x%02X: not supported", hv[0]);
    hd->mode = 0;
  } else {
    if (adobe_rgb || (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B'))
      CDN_JPEG_FAIL(kUnsupported, "RGB-coded stream: not supported");
    if (hv[1] != 0x11 || hv[2] != 0x11 || (hv[0] != 0x11 && hv[0] != 0x21 && hv[0] != 0x22))
      CDN_JPEG_FAIL(kUnsupported, "sampling %02X %02X %02X: 4:4:4, 4:2:2 and 4:2:0 are supported", hv[0], hv[1], hv[2]);
    hd->mode = hv[0] == 0x11 ? 0 : (hv[0] == 0x21 ? 1 : 2);
  }
  const int hs = hd->mode >= 1 ? 2 : 1, vs = hd->mode == 2 ? 2 : 1;
  hd->mcus_x = (hd->w + 8 * hs - 1) / (8 * hs);
  hd->mcus_y = (hd->h + 8 * vs - 1) / (8 * vs);
  // DC symbols are bit counts
  for (int t = 0; t < 2; ++t)
    for (int i = 0; hd->have_h[t] && i < 256; ++i)
      if (hd->vals[t][i] > 15) CDN_JPEG_FAIL(kMalformed, "DC Huffman symbol %d", hd->vals[t][i]);
  // the segments: one more than the restart markers
  struct Count {
    int rst = 0;
    int operator()(int kind, const uint8_t *, int64_t) {
      rst += kind == 2;
      return 0;
    }
  } count;
  const int rc = walk_scan(d, n, hd->scan_off, count, msg, msg_len);
  if (rc) return rc;
  hd->n_segments = expected_segments(*hd);
  if (count.rst && hd->restart == 0) CDN_JPEG_FAIL(kMalformed, "restart marker without a restart interval");
  if (count.rst + 1 > hd->n_segments) CDN_JPEG_FAIL(kMalformed, "%d restart markers for %d intervals", count.rst, hd->n_segments);
  return kParsed;
}

// decode form of a table (jdhuff.c: jpeg_make_d_derived_tbl); false: the counts do not describe a prefix code
inline bool derive_huff(const uint8_t *bits, const uint8_t *vals, Huff *t) {
  memset(t, 0, sizeof(*t));
  int size[257], code_of[257], p = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < bits[l]; ++i) {
      if (p >= 256) return false;
      size[p++] = l;
    }
  const int nsym = p;
  size[p] = 0;
  int code = 0, si = nsym ? size[0] : 0;
  p = 0;
  while (p < nsym) {
    while (p < nsym && size[p] == si) code_of[p++] = code++;
    if (code > (1 << si)) return false;
    code <<= 1;
    ++si;
  }
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (bits[l]) {
      t->valoff[l] = p - code_of[p];
      p += bits[l];
      t->maxcode[l] = code_of[p - 1];
    } else {
      t->maxcode[l] = -1;
    }
  }
  t->maxcode[0] = -1;
  p = 0;
  for (int l = 1; l <= 9; ++l)
    for (int i = 0; i < bits[l]; ++i, ++p) {
      const int first = code_of[p] << (9 - l);
      for (int k = 0; k < (1 << (9 - l)); ++k) t->look[first + k] = (uint16_t)((l << 8) | vals[p]);
    }
  memcpy(t->huffval, vals, 256);
  return true;
}

// where pack() writes: host buffers and how much of each is used
struct PackTarget {
  uint8_t *stream;
  int64_t stream_used, stream_cap;
  int32_t *segs;                    // header record + seg_cap records
  int64_t segs_used, seg_cap;
  int32_t *item_rec;                // this item's record
  uint8_t *tables;                  // this item's blob
  int64_t plane_stride;
};
enum { kWorkspace = -6 };           // (CDN_ERR_WORKSPACE)

inline int pack(const uint8_t *d, int64_t n, int item, int64_t out_off, int64_t out_pitch, PackTarget *tg, char *msg,
                size_t msg_len) {
  Header hd;
  const int rc = parse(d, n, &hd, msg, msg_len);
  if (rc) return rc;
  const int hs = hd.mode >= 1 ? 2 : 1, vs = hd.mode == 2 ? 2 : 1;
  int32_t rec[kItemWords] = {0};
  rec[kW] = hd.w;
  rec[kH] = hd.h;
  rec[kNComp] = hd.ncomp;
  rec[kMode] = hd.mode;
  rec[kMcusX] = hd.mcus_x;
  rec[kMcusY] = hd.mcus_y;
  for (int c = 0; c < hd.ncomp; ++c) rec[kSel] |= (hd.td[c] << (2 * c)) | (hd.ta[c] << (2 * c + 1));
  rec[kPitchY] = hd.mcus_x * 8 * hs;
  rec[kRowsY] = hd.mcus_y * 8 * vs;
  rec[kPitchC] = hd.mcus_x * 8;
  rec[kRowsC] = hd.mcus_y * 8;
  rec[kRestart] = hd.restart;
  rec[kOutLo] = (int32_t)(uint32_t)((uint64_t)out_off & 0xffffffffu);
  rec[kOutHi] = (int32_t)(uint32_t)((uint64_t)out_off >> 32);
  rec[kOutPitch] = (int32_t)out_pitch;
  Geom g;
  if (out_off < 0 || out_pitch < 3 * (int64_t)hd.w || out_pitch > 0x7fffffff)
    CDN_JPEG_FAIL(kMalformed, "output offset %lld / pitch %lld for width %d", (long long)out_off, (long long)out_pitch, hd.w);
  if (!item_geom(rec, tg->plane_stride, &g))
    CDN_JPEG_FAIL(kWorkspace, "a %d x %d image is beyond the plane capacity of %lld bytes per item", hd.w, hd.h,
                  (long long)tg->plane_stride);
  if (tg->segs_used + hd.n_segments > tg->seg_cap)
    CDN_JPEG_FAIL(kWorkspace, "%lld segments are beyond the capacity of %lld", (long long)(tg->segs_used + hd.n_segments),
                  (long long)tg->seg_cap);
  // the entropy-coded bytes shrink or keep their length: checked once, before the first byte is written
  if (tg->stream_used + (n - hd.scan_off) > tg->stream_cap || tg->stream_used + (n - hd.scan_off) > 0x7fffffff)
    CDN_JPEG_FAIL(kWorkspace, "%lld stream bytes are beyond the capacity of %lld", (long long)(tg->stream_used + n - hd.scan_off),
                  (long long)tg->stream_cap);
  Tables *tab = reinterpret_cast<Tables *>(tg->tables);
  memset(tab, 0, sizeof(*tab));
  for (int c = 0; c < hd.ncomp; ++c) memcpy(tab->quant[c], hd.quant[hd.tq[c]], 64);
  for (int k = 0; k < 64; ++k) tab->zigzag[k] = (uint8_t)zigzag(k);
  for (int t = 0; t < 4; ++t) {
    if (hd.have_h[t]) {
      if (!derive_huff(hd.bits[t], hd.vals[t], &tab->huff[t])) CDN_JPEG_FAIL(kMalformed, "Huffman table %d is not a prefix code", t);
    } else {
      for (int l = 0; l <= 16; ++l) tab->huff[t].maxcode[l] = -1;
    }
  }
  const int total = total_mcus(hd), per = hd.restart > 0 ? hd.restart : total;
  struct Sink {
    PackTarget *tg;
    int64_t seg_start;
    int nseg = 0, item, per, total, limit;
    void close() {
      if (nseg >= limit) return;
      int32_t *r = tg->segs + (1 + tg->segs_used + nseg) * kSegWords;
      const int first = nseg * per;
      r[kSegItem] = item;
      r[kSegFirst] = first;
      r[kSegCount] = total - first < per ? total - first : per;
      r[kSegOff] = (int32_t)seg_start;
      r[kSegLen] = (int32_t)(tg->stream_used - seg_start);
      r[5] = r[6] = r[7] = 0;
      ++nseg;
      seg_start = tg->stream_used;
    }
    int operator()(int kind, const uint8_t *p, int64_t k) {
      if (kind == 0) {
        memcpy(tg->stream + tg->stream_used, p, (size_t)k);
        tg->stream_used += k;
      } else if (kind == 1) {
        tg->stream[tg->stream_used++] = 0xFF;
      } else {
        close();
      }
      return 0;
    }
  } sink;
  sink.tg = tg;
  sink.seg_start = tg->stream_used;
  sink.item = item;
  sink.per = per;
  sink.total = total;
  sink.limit = hd.n_segments;
  const int rw = walk_scan(d, n, hd.scan_off, sink, msg, msg_len);
  if (rw) return rw;        // (parse walked the same bytes: not reached)
  // the last segment ends at EOI or at the end of the data; segments a truncated stream never reached are empty
  while (sink.nseg < hd.n_segments) sink.close();
  tg->segs_used += hd.n_segments;
  memcpy(tg->item_rec, rec, sizeof(rec));
  tg->segs[0] = (int32_t)tg->segs_used;
  tg->segs[1] = item + 1;
  for (int k = 2; k < kSegWords; ++k) tg->segs[k] = 0;
  return kParsed;
}

}  // namespace cdn_jpeg
