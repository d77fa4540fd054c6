// jpeg_host_fuzz.cpp -- the JPEG decoder core (codenet_amd/csrc/cdn_jpeg.h: parse, pack, the segment decoder, up-sampling
// and colour -- the text the GPU kernels run) on corrupt streams, on the host, under AddressSanitizer and
// UndefinedBehaviorSanitizer.  Plain C++ with its own main; no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o build/jpeg_host_fuzz tools/probes/jpeg_host_fuzz.cpp
//   build/jpeg_host_fuzz tests/golden/jpeg_fuzz_420.jpg tests/golden/jpeg_fuzz_444_r3.jpg \
//       tests/golden/jpeg_fuzz_420_q100.jpg
//
// (a 4:2:0 stream, one with a restart interval of 3 MCUs, and one whose single segment is longer than the decoder's 2 KB
// stream window, so that the window is refilled)
//
// Per input file: the intact stream (status 0 expected), a truncation at every 7th byte of the entropy-coded data, 200
// seeded single-bit flips in it, and 10 000 seeded random corruptions of the whole file (bit flips, overwritten runs,
// inserted markers, truncations; the header included).  Every buffer is a heap block of exactly the size the library is
// told, and the output and plane buffers carry 64 guard bytes on either side inside that block which must stay intact.
// Every stream that reaches the decoder is also decoded by the parallel entropy path (decode_host_parallel) with
// sub-sequences of 64 and of 1024 bits, its coefficient workspace guarded in the same way: its status must be zero
// exactly when the serial status is zero, and then its pixels must be the serial pixels.
// Exit status 0: every call returned, no guard byte changed and the two paths agreed; the sanitizers abort on anything
// else.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codenet_amd/csrc/cdn_jpeg.h"

namespace J = cdn_jpeg;

namespace {

constexpr int kGuard = 64;
constexpr int kMaxSide = 128;       // capacity: header corruptions that ask for more are refused by pack()

struct Rng {
  uint64_t s;
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)(s >> 16);
  }
  uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

struct Tally {
  long runs = 0, refused = 0, clean = 0, flagged = 0, parallel = 0, disagreed = 0;
};

bool guards_intact(const std::vector<uint8_t> &b) {
  for (int k = 0; k < kGuard; ++k)
    if (b[k] != 0xA5 || b[b.size() - 1 - k] != 0xA5) return false;
  return true;
}

// parse + pack + decode of one (possibly corrupt) file; false: a guard byte changed
bool run_one(const std::vector<uint8_t> &d, Tally *t, int *status_out = nullptr) {
  ++t->runs;
  char msg[200];
  J::Header hd;
  if (J::parse(d.data(), (int64_t)d.size(), &hd, msg, sizeof(msg)) != J::kParsed) {
    ++t->refused;
    return true;
  }
  const int64_t stride = J::plane_stride(kMaxSide, kMaxSide);
  // 16-byte alignment of the blob and 8 of the planes: operator new gives 16, the guard keeps it
  std::vector<uint8_t> stream(d.size() - (size_t)hd.scan_off + 1), tables(J::kTableBytes);
  std::vector<int32_t> segs((size_t)(1 + hd.n_segments) * J::kSegWords), item(J::kItemWords), status(1, 0);
  J::PackTarget tg{stream.data(), 0, (int64_t)stream.size(), segs.data(), 0, hd.n_segments, item.data(), tables.data(), stride};
  if (J::pack(d.data(), (int64_t)d.size(), 0, 0, 3 * (int64_t)hd.w, &tg, msg, sizeof(msg)) != J::kParsed) {
    ++t->refused;
    return true;
  }
  const int64_t out_bytes = (int64_t)hd.w * hd.h * 3;
  std::vector<uint8_t> out((size_t)out_bytes + 2 * kGuard, 0xA5), planes((size_t)stride + 2 * kGuard, 0xA5);
  J::Call c{stream.data(), (int64_t)stream.size(), segs.data(), hd.n_segments, item.data(), 1, tables.data(),
            planes.data() + kGuard, stride, status.data(), out.data() + kGuard, out_bytes, 0};
  J::decode_host(c);
  status[0] ? ++t->flagged : ++t->clean;
  if (status_out) *status_out = status[0];
  bool ok = guards_intact(out) && guards_intact(planes);
  for (int bits : {64, 1024}) {     // the parallel entropy path on the same records
    const int64_t work_bytes = J::par_work_stride(stride);
    std::vector<uint8_t> out2(out.size(), 0xA5), planes2(planes.size(), 0xA5);
    uint8_t *raw = static_cast<uint8_t *>(aligned_alloc(16, (size_t)work_bytes + 2 * kGuard));       // (kGuard keeps the 16)
    std::vector<int32_t> status2(1, 0);
    memset(raw, 0xA5, (size_t)work_bytes + 2 * kGuard);
    J::ParCall pc{c, raw + kGuard, work_bytes, bits};
    pc.c.planes = planes2.data() + kGuard;
    pc.c.out = out2.data() + kGuard;
    pc.c.status = status2.data();
    J::decode_host_parallel(pc);
    ++t->parallel;
    for (int k = 0; k < kGuard; ++k) ok = ok && raw[k] == 0xA5 && raw[kGuard + work_bytes + k] == 0xA5;
    free(raw);
    ok = ok && guards_intact(out2) && guards_intact(planes2);
    if ((status2[0] != 0) != (status[0] != 0) || (status[0] == 0 && out2 != out)) {
      ++t->disagreed;
      ok = false;
    }
  }
  return ok;
}

std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> d;
  FILE *f = fopen(path, "rb");
  if (!f) return d;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
  fclose(f);
  return d;
}

int fuzz_file(const char *path) {
  const std::vector<uint8_t> good = read_file(path);
  char msg[200];
  J::Header hd;
  if (good.empty() || J::parse(good.data(), (int64_t)good.size(), &hd, msg, sizeof(msg)) != J::kParsed) {
    fprintf(stderr, "%s: cannot read or parse\n", path);
    return 1;
  }
  const size_t scan = (size_t)hd.scan_off, n = good.size();
  Tally t;
  int st = -1;
  bool ok = run_one(good, &t, &st);
  if (st != 0) {
    fprintf(stderr, "%s: the intact stream decodes with status %d\n", path, st);
    return 1;
  }
  for (size_t cut = scan; cut < n && ok; cut += 7) ok = run_one(std::vector<uint8_t>(good.begin(), good.begin() + cut), &t);
  Rng rng{0x9E3779B97F4A7C15ull};
  for (int k = 0; k < 200 && ok; ++k) {
    std::vector<uint8_t> d = good;
    d[scan + rng.below((uint32_t)(n - scan))] ^= (uint8_t)(1u << rng.below(8));
    ok = run_one(d, &t);
  }
  for (int k = 0; k < 10000 && ok; ++k) {
    std::vector<uint8_t> d = good;
    const uint32_t kind = rng.below(8);
    // three in eight corrupt the header too; the rest keep it so that the decoder itself sees the damage
    const size_t lo = kind < 3 ? 2 : scan;
    const int edits = 1 + (int)rng.below(4);
    for (int e = 0; e < edits; ++e) {
      const size_t at = lo + rng.below((uint32_t)(d.size() - lo));
      switch (rng.below(5)) {
        case 0:
          d[at] ^= (uint8_t)(1u << rng.below(8));
          break;
        case 1:
          for (size_t j = at, end = at + 1 + rng.below(16); j < end && j < d.size(); ++j) d[j] = (uint8_t)rng.next();
          break;
        case 2:
          d[at] = 0xFF;
          if (at + 1 < d.size()) d[at + 1] = (uint8_t)(rng.below(2) ? 0xD0 + rng.below(8) : rng.next());
          break;
        case 3:
          for (size_t j = at, end = at + 1 + rng.below(64); j < end && j < d.size(); ++j) d[j] = rng.below(2) ? 0x00 : 0xFF;
          break;
        default:
          if (at > lo + 1) d.resize(at);
          break;
      }
    }
    ok = run_one(d, &t);
  }
  printf("%s: %ld runs, %ld refused by parse / pack, %ld decoded with status 0, %ld with a non-zero status, %ld parallel "
         "decodes of which %ld disagreed with the serial one, guards %s\n",
         path, t.runs, t.refused, t.clean, t.flagged, t.parallel, t.disagreed, ok ? "intact" : "DAMAGED");
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg [file.jpg ...]\n", argv[0]);
    return 2;
  }
  int rc = 0;
  for (int k = 1; k < argc; ++k) rc |= fuzz_file(argv[k]);
  return rc;
}
