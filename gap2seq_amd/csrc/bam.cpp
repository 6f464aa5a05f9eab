// gap2seq_amd/csrc/bam.cpp — see bam.hpp.
#include "bam.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "bam_rows.h"
#include "bam_store.h"
#include "bgzf_inflate.h"
#include "inflate_core.h"

namespace g2s {

namespace {
inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }  // (little-endian host)
// inflated bytes per refill (G2S_BAM_CHUNK: the tests make it small so that records span refills), read when a
// pass over the file begins
size_t chunk_bytes() {
  const char* e = getenv("G2S_BAM_CHUNK");
  const long long n = e ? atoll(e) : 0;
  return n > 0 ? (size_t)n : (size_t)32 << 20;
}
// device path: room in front of a page-locked window for the bytes carried over from the window before
constexpr size_t kDeviceFront = (size_t)256 << 10;
}  // namespace

BamFile::~BamFile() {
  if (map_) munmap(map_, map_len_);
}

bool BamFile::open_path(const std::string& path, std::string* err) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) { *err = "cannot open " + path; return false; }
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size <= 0) { ::close(fd); *err = "cannot read " + path; return false; }
  void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (m == MAP_FAILED) { *err = "cannot map " + path; return false; }
  map_ = m;
  map_len_ = (size_t)st.st_size;
  madvise(m, map_len_, MADV_SEQUENTIAL);
  return open_mem(m, map_len_, err);
}

bool BamFile::open_mem(const void* bytes, size_t n, std::string* err) {
  data_ = (const uint8_t*)bytes;
  size_ = n;
  return index_blocks(err) && read_header(err);
}

// BGZF (SAM specification 4.1): gzip members with an extra subfield 'B','C' holding the member's size - 1
bool BamFile::index_blocks(std::string* err) {
  blk_off_.clear(); blk_csize_.clear(); blk_isize_.clear(); blk_dataoff_.clear();
  size_t o = 0;
  while (o < size_) {
    if (o + 18 > size_ || data_[o] != 0x1f || data_[o + 1] != 0x8b || data_[o + 2] != 8 || !(data_[o + 3] & 4)) {
      *err = "not a BGZF file (block " + std::to_string(blk_off_.size()) + ")";
      return false;
    }
    const size_t xlen = rd16(data_ + o + 10);
    if (o + 12 + xlen > size_) { *err = "truncated BGZF header"; return false; }
    size_t bsize = 0;
    for (size_t x = o + 12; x + 4 <= o + 12 + xlen;) {
      const size_t slen = rd16(data_ + x + 2);
      if (data_[x] == 'B' && data_[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) bsize = (size_t)rd16(data_ + x + 4) + 1;
      x += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || o + bsize > size_) { *err = "truncated BGZF block"; return false; }
    const uint32_t isize = rd32(data_ + o + bsize - 4);
    if (isize > 65536) { *err = "BGZF block larger than 64 KiB"; return false; }
    blk_off_.push_back(o);
    blk_csize_.push_back((uint32_t)bsize);
    blk_isize_.push_back(isize);
    blk_dataoff_.push_back((uint16_t)(12 + xlen));
    o += bsize;
  }
  if (blk_off_.empty()) { *err = "empty file"; return false; }
  return true;
}

// the inflated stream, a window at a time
struct BamFile::Stream {
  const BamFile& f;
  size_t next_blk = 0;
  std::vector<uint8_t> buf;        // the host path's window
  const uint8_t* base = nullptr;   // where [lo, hi) is: buf, or a page-locked window of the device path read in place
  size_t lo = 0, hi = 0;
  std::string err;
  int64_t bad_blk = -1;
  const size_t chunk = f.window_bytes_ ? f.window_bytes_ : chunk_bytes();
  // device path: the slot whose window is being read, and the window in flight
  BgzfDevice* dev = nullptr;
  int cur = -1, fly = -1;
  size_t fly_end = 0, fly_beg = 0, fly_bytes = 0, fly_in = 0;
  explicit Stream(const BamFile& file) : f(file) {}
  ~Stream() {
    if (dev && fly >= 0) (void)dev->wait(fly, nullptr);  // (a walk that ended early leaves its look-ahead behind)
  }

  static bool inflate_block(z_stream* zs, const BamFile& f, size_t b, uint8_t* out) {
    const uint8_t* blk = f.data_ + f.blk_off_[b];
    const uint32_t isize = f.blk_isize_[b];
    if (isize == 0) return true;  // (the end-of-file marker, or an empty block)
    if (inflateReset(zs) != Z_OK) return false;
    zs->next_in = const_cast<Bytef*>(blk + f.blk_dataoff_[b]);
    zs->avail_in = f.blk_csize_[b] - f.blk_dataoff_[b] - 8;
    zs->next_out = out;
    zs->avail_out = isize;
    if (::inflate(zs, Z_FINISH) != Z_STREAM_END || zs->avail_out != 0) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, isize) == rd32(blk + f.blk_csize_[b] - 8);
  }
  // the same with inflate_core.h, CRC by slices as the kernel computes it (set_inflate_core: tests)
  static bool inflate_block_core(const BamFile& f, size_t b, uint8_t* out) {
    const uint8_t* blk = f.data_ + f.blk_off_[b];
    const uint32_t isize = f.blk_isize_[b];
    if (isize == 0) return true;
    inflate::Tables T;
    inflate::HostSink sink{out};
    if (inflate::inflate_member(blk + f.blk_dataoff_[b], f.blk_csize_[b] - f.blk_dataoff_[b] - 8, isize, &T, sink) != inflate::kOk)
      return false;
    return inflate::crc_by_slices(out, isize) == rd32(blk + f.blk_csize_[b] - 8);
  }

  // the members [b0, e) of the window that starts at b0, and their inflated bytes
  size_t window_end(size_t b0, size_t* bytes) const {
    const size_t nb = f.blk_off_.size();
    size_t e = b0;
    *bytes = 0;
    while (e < nb && (e == b0 || *bytes + f.blk_isize_[e] <= chunk)) *bytes += f.blk_isize_[e++];
    return e;
  }

  bool refill() {
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = refill_window();
    f.stats_.ms_refill += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ok;
  }

  bool refill_window() {
    const size_t nb = f.blk_off_.size();
    if (next_blk >= nb || !err.empty()) return false;
    if (f.inflate_device_ >= 0 && !f.dev_refused_) {
      const int r = refill_device();
      if (r >= 0) return r == 1;
    }
    const size_t left = hi - lo;
    if (base == buf.data()) {
      if (lo) memmove(buf.data(), buf.data() + lo, left);
    } else {  // (bytes left in a device window: the host path goes on from them)
      if (buf.size() < left) buf.resize(left);
      if (left) memcpy(buf.data(), base + lo, left);
    }
    lo = 0;
    hi = left;
    size_t bytes = 0;
    const size_t e = window_end(next_blk, &bytes);
    if (buf.size() < hi + bytes) buf.resize(hi + bytes);
    base = buf.data();
    std::vector<size_t> at(e - next_blk);
    for (size_t b = next_blk, o = hi; b < e; b++) { at[b - next_blk] = o; o += f.blk_isize_[b]; }
    const int T = (int)std::min<size_t>((size_t)f.threads_, std::max<size_t>(1, (e - next_blk) / 16));
    std::atomic<size_t> bad{(size_t)-1};
    auto work = [&](int t) {
      if (f.use_core_) {
        for (size_t b = next_blk + (size_t)t; b < e; b += (size_t)T)
          if (!inflate_block_core(f, b, buf.data() + at[b - next_blk])) { bad = b; break; }
        return;
      }
      z_stream zs;
      memset(&zs, 0, sizeof zs);
      if (inflateInit2(&zs, -15) != Z_OK) { bad = next_blk; return; }
      for (size_t b = next_blk + (size_t)t; b < e; b += (size_t)T)
        if (!inflate_block(&zs, f, b, buf.data() + at[b - next_blk])) { bad = b; break; }
      inflateEnd(&zs);
    };
    if (T <= 1) work(0);
    else {
      std::vector<std::thread> th;
      for (int t = 1; t < T; t++) th.emplace_back(work, t);
      work(0);
      for (auto& x : th) x.join();
    }
    if (bad.load() != (size_t)-1) {
      bad_blk = (int64_t)bad.load();
      err = "corrupt BGZF block " + std::to_string(bad.load());
      return false;
    }
    for (size_t b = next_blk; b < e; b++) f.stats_.bytes_in += f.blk_csize_[b];
    f.stats_.members += e - next_blk;
    f.stats_.bytes_out += bytes;
    f.stats_.host_windows++;
    hi += bytes;
    next_blk = e;
    return true;
  }

  // ---- the device path.  Window n is read in place from its slot's page-locked buffer while window n + 1 is on its
  // way through the other slot: staged, copied up, inflated, copied down, an event at the end.
  void refuse(const std::string& why) {
    f.dev_refused_ = true;
    if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s] BGZF inflate: the device refused (%s): zlib on the host from block %zu\n",
                                     why.c_str(), next_blk);
  }
  // (`down` false: the window stays in device memory, for rows_on_device)
  // (`d_dst`: its place in the resident stream of one-pass mode)
  bool issue(int slot, size_t b0, std::string* why, bool down = true, uint8_t* d_dst = nullptr) {
    size_t bytes = 0, in = 0, file_bytes = 0;
    const size_t e = window_end(b0, &bytes);
    for (size_t b = b0; b < e; b++) {
      if (f.blk_isize_[b]) in += ((size_t)(f.blk_csize_[b] - f.blk_dataoff_[b] - 8) + 15) & ~(size_t)15;
      file_bytes += f.blk_csize_[b];
    }
    if (!dev->fits(e - b0, in, bytes)) { *why = "a window larger than the buffers"; return false; }
    BgzfMember* M = dev->members(slot);
    uint8_t* hin = dev->in(slot);
    size_t out = 0;
    in = 0;
    for (size_t b = b0; b < e; b++) {
      const uint8_t* blk = f.data_ + f.blk_off_[b];
      const uint32_t dl = f.blk_csize_[b] - f.blk_dataoff_[b] - 8, isize = f.blk_isize_[b];
      M[b - b0] = BgzfMember{in, out, dl, isize, rd32(blk + f.blk_csize_[b] - 8), 0};
      if (isize) {
        memcpy(hin + in, blk + f.blk_dataoff_[b], dl);
        in += ((size_t)dl + 15) & ~(size_t)15;
      }
      out += isize;
    }
    if (!dev->launch(slot, e - b0, in, bytes, why, down, d_dst)) return false;
    fly = slot;
    fly_beg = b0;
    fly_end = e;
    fly_bytes = bytes;
    fly_in = file_bytes;
    return true;
  }
  // 1: a window was handed out; 0: a corrupt member (err); -1: the device refused, the host path inflates this window
  int refill_device() {
    std::string why;
    if (!dev && !(dev = f.device_buffers())) return -1;  // (device_buffers has said why)
    if (fly < 0 && !issue(cur < 0 ? 0 : 1 - cur, next_blk, &why)) { refuse(why); return -1; }
    if (!dev->wait(fly, &why)) { fly = -1; refuse(why); return -1; }
    const int slot = fly;
    fly = -1;
    const uint32_t* st = dev->status(slot);
    for (size_t i = 0; i < fly_end - fly_beg; i++)
      if (st[i] != inflate::kOk) {
        bad_blk = (int64_t)(fly_beg + i);
        err = "corrupt BGZF block " + std::to_string(fly_beg + i);
        return 0;
      }
    // the bytes of a record cut by the last window's end go in front of this one
    const size_t left = hi - lo;
    uint8_t* win = dev->window(slot);
    if (left <= dev->front()) {
      if (left) memcpy(win - left, base + lo, left);
      base = win - left;
    } else {  // (a record longer than the room in front: this window is read from the host buffer)
      if (base == buf.data()) {
        if (lo) memmove(buf.data(), buf.data() + lo, left);
        buf.resize(left + fly_bytes);
      } else {
        std::vector<uint8_t> nb(left + fly_bytes);
        memcpy(nb.data(), base + lo, left);
        buf.swap(nb);
      }
      if (fly_bytes) memcpy(buf.data() + left, win, fly_bytes);
      base = buf.data();
    }
    lo = 0;
    hi = left + fly_bytes;
    cur = slot;
    next_blk = fly_end;
    f.stats_.members += fly_end - fly_beg;
    f.stats_.bytes_in += fly_in;
    f.stats_.bytes_out += fly_bytes;
    f.stats_.device_windows++;
    if (next_blk < f.blk_off_.size() && !issue(1 - slot, next_blk, &why)) refuse(why);  // (this window is good)
    return 1;
  }

  // n contiguous bytes at the read position, or null at the end of the stream / on an error
  const uint8_t* need(size_t n) {
    while (hi - lo < n)
      if (!refill()) return nullptr;
    return base + lo;
  }
  void consume(size_t n) { lo += n; }
  bool skip(uint64_t n) {
    while (n) {
      const size_t step = (size_t)std::min<uint64_t>(n, 1 << 16);
      if (!need(step)) return false;
      consume(step);
      n -= step;
    }
    return true;
  }
  size_t left() const { return hi - lo; }
};

void BamFile::set_inflate_device(int device) {
  if (device != inflate_device_) { dev_.reset(); dev_refused_ = false; }
  inflate_device_ = device < 0 ? -1 : device;
}

size_t BamFile::largest_window(size_t* staged, size_t* members, size_t* inflated) const {
  Stream s(*this);
  size_t max_in = 0, max_out = 0, max_members = 0;
  for (size_t b = 0; b < blk_off_.size();) {
    size_t bytes = 0, in = 0;
    const size_t e = s.window_end(b, &bytes);
    for (size_t i = b; i < e; i++)
      if (blk_isize_[i]) in += ((size_t)(blk_csize_[i] - blk_dataoff_[i] - 8) + 15) & ~(size_t)15;
    max_in = std::max(max_in, in);
    max_out = std::max(max_out, bytes);
    max_members = std::max(max_members, e - b);
    b = e;
  }
  if (staged) *staged = max_in;
  if (members) *members = max_members;
  if (inflated) *inflated = max_out;
  return max_out;
}

// the buffers of the device path, sized by the file's largest window
BgzfDevice* BamFile::device_buffers() const {
  if (dev_) return dev_.get();
  size_t max_in = 0, max_out = 0, max_members = 0;
  largest_window(&max_in, &max_members, &max_out);
  std::string why;
  dev_.reset(BgzfDevice::create(inflate_device_, max_in, max_out, max_members, kDeviceFront, &why));
  if (!dev_) {
    dev_refused_ = true;
    if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s] BGZF inflate: the device refused (%s): zlib on the host\n", why.c_str());
  }
  return dev_.get();
}

bool BamFile::open_bgzf(const void* bytes, size_t n, std::string* err) {
  data_ = (const uint8_t*)bytes;
  size_ = n;
  return index_blocks(err);
}

bool BamFile::read_all(std::vector<uint8_t>* out, std::string* err, int64_t* bad_block) const {
  Stream s(*this);
  out->clear();
  while (s.refill()) {
    out->insert(out->end(), s.base + s.lo, s.base + s.hi);
    s.lo = s.hi;
  }
  if (bad_block) *bad_block = s.bad_blk;
  if (!s.err.empty()) { *err = s.err; return false; }
  return true;
}

// BAM header (SAM specification 4.2): magic, SAM text, reference names and lengths
bool BamFile::read_header(std::string* err) {
  Stream s(*this);
  auto fail = [&](const char* what) { *err = s.err.empty() ? what : s.err; return false; };
  const uint8_t* p = s.need(12);
  if (!p || memcmp(p, "BAM\1", 4) != 0) return fail("not a BAM file");
  const uint32_t l_text = rd32(p + 4);
  s.consume(8);
  uint64_t used = 8;
  if (!s.skip(l_text)) return fail("truncated BAM header");
  used += l_text;
  p = s.need(4);
  if (!p) return fail("truncated BAM header");
  const uint32_t n_ref = rd32(p);
  s.consume(4);
  used += 4;
  ref_names_.clear();
  for (uint32_t r = 0; r < n_ref; r++) {
    p = s.need(4);
    if (!p) return fail("truncated BAM header");
    const uint32_t l_name = rd32(p);
    if (l_name == 0 || l_name > (1u << 20)) return fail("bad reference name in the BAM header");
    p = s.need(4 + (size_t)l_name + 4);
    if (!p) return fail("truncated BAM header");
    ref_names_.emplace_back((const char*)p + 4, strnlen((const char*)p + 4, l_name));
    s.consume(4 + (size_t)l_name + 4);
    used += 4 + (uint64_t)l_name + 4;
  }
  first_rec_ = used;
  return true;
}

int BamFile::ref_id(const std::string& name) const {
  for (size_t i = 0; i < ref_names_.size(); i++)
    if (ref_names_[i] == name) return (int)i;
  return -1;
}

bool BamFile::for_each(const std::function<bool(const BamRec&)>& fn, std::string* err) const {
  Stream s(*this);
  auto fail = [&](const char* what) { *err = s.err.empty() ? what : s.err; return false; };
  if (!s.skip(first_rec_)) return fail("truncated BAM header");
  for (;;) {
    const uint8_t* p = s.need(4);
    if (!p) {
      if (!s.err.empty() || s.left() != 0) return fail("truncated BAM record");
      return true;
    }
    const uint32_t bs = rd32(p);
    if (bs < 32 || bs > (1u << 30)) return fail("bad BAM record size");
    p = s.need(4 + (size_t)bs);
    if (!p) return fail("truncated BAM record");
    p += 4;
    BamRec r;
    r.ref_id = (int32_t)rd32(p);
    r.pos = (int32_t)rd32(p + 4);
    r.l_name = p[8];
    r.mapq = p[9];
    r.n_cigar = rd16(p + 12);
    r.flag = rd16(p + 14);
    r.l_seq = (int32_t)rd32(p + 16);
    r.next_ref_id = (int32_t)rd32(p + 20);
    r.next_pos = (int32_t)rd32(p + 24);
    r.tlen = (int32_t)rd32(p + 28);
    if (r.l_seq < 0 || r.l_name == 0 ||
        32 + (uint64_t)r.l_name + 4 * (uint64_t)r.n_cigar + ((uint64_t)r.l_seq + 1) / 2 + (uint64_t)r.l_seq > bs)
      return fail("bad BAM record layout");
    r.name = (const char*)p + 32;
    r.cigar = p + 32 + r.l_name;
    r.seq = r.cigar + 4 * (size_t)r.n_cigar;
    if (!fn(r)) return true;
    s.consume(4 + (size_t)bs);
  }
}

bool BamFile::store_sample(uint64_t sample, StorePlan* plan, std::string* err) const {
  const uint64_t total = inflated_bytes(), P = total > first_rec_ ? total - first_rec_ : 0;
  const uint64_t lim = first_rec_ + std::min<uint64_t>(sample ? sample : kStoreSampleBytes, P);
  const uint64_t want = std::min<uint64_t>(total, lim + bam_store::kHead);  // (the head of a record that begins at the sample's last byte)
  std::vector<uint8_t> buf;
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) { *err = "zlib"; return false; }
  for (size_t b = 0; b < blk_off_.size() && buf.size() < want; b++) {
    const size_t at = buf.size();
    buf.resize(at + blk_isize_[b]);
    if (!Stream::inflate_block(&zs, *this, b, buf.data() + at)) {
      inflateEnd(&zs);
      *err = "corrupt BGZF block " + std::to_string(b);
      return false;
    }
  }
  inflateEnd(&zs);
  uint64_t r = 0, c = 0, o = first_rec_;
  while (o < lim && o + bam_store::kHead <= buf.size()) {
    const uint8_t* rec = buf.data() + o;
    const uint32_t bs = rd32(rec), l_name = rec[12];
    const int32_t l_seq = (int32_t)rd32(rec + 20);
    if (bs < 32 || bs > (1u << 30) || l_seq < 0 || l_name == 0) break;  // (the pass itself says what is wrong with it)
    r++;
    c += bam_store::stored_bytes(l_name, (uint64_t)l_seq);
    o += 4 + (uint64_t)bs;
  }
  *plan = store_plan(P, r, std::min(o, total) - first_rec_, c);
  return true;
}

bool BamFile::store_on_host(std::vector<uint8_t>* store, std::vector<uint64_t>* rec_off, std::string* err) const {
  store->clear();
  rec_off->clear();
  return for_each([&](const BamRec& r) {
    rec_off->push_back(store->size());
    bam_store::append_record((const uint8_t*)r.name - bam_store::kHead, store);
    return true;
  }, err);
}

uint64_t BamFile::inflated_bytes() const {
  uint64_t total = 0;
  for (const uint32_t isize : blk_isize_) total += isize;
  return total;
}

uint64_t BamFile::inflate_device_bytes() const {
  size_t max_in = 0, max_out = 0, max_members = 0;
  largest_window(&max_in, &max_members, &max_out);
  return BgzfDevice::device_bytes(max_in, max_out, max_members, kDeviceFront);
}

// Pass A without the walk: every window is inflated into its slot's device buffer and left there, and the row kernels
// (bam_rows.hip) follow the inflate kernel on the same stream; the host stages window n + 1 while window n is on the
// device, and looks at a window's member status two windows later, when its slot is needed again.
// One-pass mode (`resident`): the windows are inflated into one allocation, each at its inflated offset, and stay there
// for pass B (bam_text.hip).  A window's base is then no word boundary in general, so the row kernels are given the
// word boundary in front of it and start that many bytes in; a record cut by a window's end is whole in memory, and in
// place of the carry the chain's head moves by the distance between the two bases (BamRowsDevice::advance).
// The streaming form (`sink`): the two slots as without `resident`, the rows compact and consumed window by window.
// The store route (`store`): the two slots as without `resident`, whole-file rows of the planned count, and the store's
// kernels behind the row kernels of every walk window (BamRowsDevice::window).
BamRowsDevice* BamFile::rows_on_device(size_t walk_window, int* anomaly, std::string* why, bool resident, uint64_t resident_cap,
                                       int* resident_refused, const RowsSink* sink, const StoreAsk* store) const {
  const auto t0 = std::chrono::steady_clock::now();
  *anomaly = kRowsHip;
  store_report_ = StoreReport();
  if (inflate_device_ < 0 || dev_refused_) { *why = "the reader does not inflate on a device"; return nullptr; }
  Stream s(*this);
  if (!(s.dev = device_buffers())) { *why = "no device buffers"; return nullptr; }
  BgzfDevice* dev = s.dev;
  const size_t nb = blk_off_.size();
  uint64_t total = 0;
  size_t max_out = 0, first_bytes = 0;
  for (size_t b = 0; b < nb;) {
    size_t bytes = 0;
    const size_t e = s.window_end(b, &bytes);
    if (b == 0) first_bytes = bytes;
    total += bytes;
    max_out = std::max(max_out, bytes);
    b = e;
  }
  const uint64_t cap_rows = total / 36 + 1;
  if (sink) resident = false;
  const bool may_store = resident && store && store->mode != 0;  // (the row limit then applies to the planned rows)
  const bool rows_fit = sink || cap_rows < (uint64_t)UINT32_MAX - 1;
  if (first_rec_ > first_bytes || max_out + dev->front() + 64 >= (size_t)INT32_MAX || (!rows_fit && !may_store)) {
    *anomaly = kRowsLimits;
    *why = "a header beyond the first window, or a file outside the row kernels' index widths";
    return nullptr;
  }
  ResidentAsk ask;
  ask.bytes = resident ? total : 0;
  ask.cap = resident_cap;
  if (may_store) {
    const StoreAsk sa = *store;
    const uint64_t P = total - first_rec_;
    ask.store = sa.mode;
    ask.plan = [this, sa, P](StorePlan* p) {
      if (sa.worst_case) {
        *p = StorePlan();
        p->rows_cap = P / 36 + 1, p->store_cap = P, p->need = 52 * (p->rows_cap + 1) + P;
        return true;
      }
      std::string e;
      return store_sample(sa.sample, p, &e);
    };
  }
  int refused = kResidentKept;
  std::unique_ptr<BamRowsDevice> R(BamRowsDevice::create(inflate_device_, dev->stream(), max_out, walk_window, dev->front(),
                                                         cap_rows, (int32_t)ref_names_.size(), first_rec_, why, &ask, &refused, sink));
  if (resident_refused) *resident_refused = refused;
  if (!R) {
    if (!rows_fit) *anomaly = kRowsLimits;
    return nullptr;
  }
  uint8_t* const keep = R->store_form() ? nullptr : R->stream_buffer();  // (null: the two slots)
  uint64_t off = 0;                          // inflated offset of the window at hand
  size_t used_beg[2] = {0, 0}, used_end[2] = {0, 0};
  // the members of the window that went through `slot` last: 0, or the anomaly
  auto settle = [&](int slot) -> int {
    if (used_end[slot] == used_beg[slot]) return kRowsOk;
    if (!dev->wait(slot, why)) return kRowsHip;
    const uint32_t* st = dev->status(slot);
    for (size_t i = 0; i < used_end[slot] - used_beg[slot]; i++)
      if (st[i] != inflate::kOk) {
        *why = "corrupt BGZF block " + std::to_string(used_beg[slot] + i);
        return kRowsCorrupt;
      }
    used_end[slot] = used_beg[slot];
    return kRowsOk;
  };
  InflateStats is;
  size_t last_bytes = 0;
  int a = kRowsOk;
  bool ok = true;
  for (size_t b = 0, w = 0; b < nb && ok; w++) {
    const int slot = (int)(w & 1);
    if ((a = settle(slot)) != kRowsOk) { ok = false; break; }
    a = kRowsHip;
    if (!s.issue(slot, b, why, false, keep ? keep + off : nullptr)) { ok = false; break; }
    used_beg[slot] = s.fly_beg;
    used_end[slot] = s.fly_end;
    b = s.fly_end;
    if (keep) {
      const uint64_t base = off & ~(uint64_t)3, next = (off + s.fly_bytes) & ~(uint64_t)3;
      const size_t lead = (size_t)(off - base);
      ok = R->window(keep + base, w == 0 ? (size_t)first_rec_ : lead, lead + s.fly_bytes, why, base);
      if (ok && b < nb) ok = R->advance(lead + s.fly_bytes, (size_t)(next - base), why);
      last_bytes = lead + s.fly_bytes;
      off += s.fly_bytes;
    } else {
      ok = R->window(dev->device_window(slot), w == 0 ? (size_t)first_rec_ : 0, s.fly_bytes, why);
      if (ok && b < nb) ok = R->carry(dev->device_window(slot), s.fly_bytes, dev->device_window(1 - slot), why);
      last_bytes = s.fly_bytes;
    }
    is.members += s.fly_end - s.fly_beg;
    is.bytes_in += s.fly_in;
    is.bytes_out += s.fly_bytes;
    is.device_windows++;
    a = kRowsOk;
  }
  for (int slot = 0; slot < 2 && ok; slot++)
    if ((a = settle(slot)) != kRowsOk) ok = false;
  if (ok) {
    a = kRowsHip;
    ok = R->finish(last_bytes, &a, why) && a == kRowsOk;
    if (a != kRowsOk && why->empty()) *why = "the row kernels met anomaly " + std::to_string(a);
  }
  if (R->store_form()) store_report_ = R->store_report();
  if (!ok) {  // (nothing of this pass is left in flight when the host walk takes the buffers over)
    (void)dev->wait(0, nullptr);
    (void)dev->wait(1, nullptr);
    *anomaly = a == kRowsOk ? (int)kRowsHip : a;
    rows_windows_ = R->windows();
    return nullptr;
  }
  *anomaly = kRowsOk;
  rows_windows_ = R->windows();
  stats_.members += is.members;
  stats_.bytes_in += is.bytes_in;
  stats_.bytes_out += is.bytes_out;
  stats_.device_windows += is.device_windows;
  stats_.ms_refill += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return R.release();
}

}  // namespace g2s
