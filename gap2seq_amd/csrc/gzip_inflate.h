// gap2seq_amd/csrc/gzip_inflate.h — a plain gzip file (any members, no BGZF) inflated chunk by chunk: the route around
// gzip_chunks.h.  gzip_route() walks the file's members and windows; a GzipBackend runs a window's four steps, on the
// device (gzip_inflate.hip: k_gz_find, k_gz_decode, k_gz_chain, k_gz_resolve, k_gz_crc) or with the same header compiled
// for the host.  The route either completes a file — every chunk ended ok, every boundary met, every member's CRC-32 and
// ISIZE matched, the end of the file or another gzip header behind every member — or gives it back with an outcome:
// zlib stays the authority on everything else, a damaged file included.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>

namespace g2s {

// why the route gave a file back (g2s_test_last_reads_gzip, g2s_test_gzip_inflate)
enum GzipOutcome : int {
  kGzDone = 0,
  kGzTooFewStarts = 1,  // a window without a second start, or (the loader) fewer starts than a quarter of the chunks
  kGzMismatch = 2,      // a chunk ran past the next start without a block boundary there: that start was a false one
  kGzSlotFull = 3,      // a chunk gave more symbols than its slot holds (G2S_GZIP_SLOT_RATIO)
  kGzCorrupt = 4,       // a chunk's decoder met what is no deflate stream, or a marker points in front of its member
  kGzTrailer = 5,       // a member's CRC-32 or ISIZE, or its trailer is cut
  kGzMemory = 6,        // the window's buffers do not fit the loader's bound
  kGzHip = 7,           // an allocation or a HIP call failed
  kGzHeader = 8,        // a member header the host parse does not take, or other bytes behind a member
};

struct GzipParams {
  uint32_t chunk = 256u << 10;  // compressed bytes a chunk (G2S_GZIP_CHUNK_BYTES)
  uint32_t window_chunks = 256; // chunks a window (G2S_GZIP_WINDOW_CHUNKS): a wave a chunk, and 256 CUs hold 512 of them
  uint32_t ratio = 8;           // a chunk's slot holds chunk * ratio symbols (G2S_GZIP_SLOT_RATIO)
  bool quarter_rule = false;    // the loader's: give back a file with fewer found starts than a quarter of its chunks
};

struct GzipStats {
  uint64_t files = 0, windows = 0, chunks = 0, starts_found = 0, absorbed = 0, members = 0, peak_device_bytes = 0;
  int outcome = kGzDone;
};

// one window's result
struct GzipWindow {
  int outcome = kGzDone;
  uint32_t jobs = 0, found = 0, covered = 0;  // chunks decoded, starts found behind the first, chunks of the window they cover
  uint64_t out_n = 0;
  uint32_t crc = 0;     // the finished CRC-32 of the window's bytes
  bool final = false;   // the member ended in this window: end_byte is the byte behind its last block
  uint64_t end_byte = 0, next_bit = 0;  // (not final: the bit of the window's bytes at which the next window begins)
};

// What runs a window.  comp[0, n): the window's compressed bytes, its first block at bit start_bit (< 8); first: the
// member begins here (no history), else the backend holds the 32 768 bytes in front from its last window, `valid` of
// them the member's; to_end: the bytes reach the file's end, so the last chunk must meet the final block.  The resolved
// bytes stand at out() + front afterwards (front: 0 or 1, the loader's held-back byte goes in front of them), in the
// backend's memory — the device's or the host's.
class GzipBackend {
 public:
  virtual ~GzipBackend() {}
  GzipWindow window(const uint8_t* comp, size_t n, uint32_t start_bit, bool first, uint32_t valid, bool to_end,
                    const GzipParams& P, uint32_t nchunks, uint32_t front);
  virtual const uint8_t* out() const = 0;
  virtual uint64_t device_bytes() const { return 0; }
  std::string why;  // (kGzHip)

 protected:
  struct Job {  // (the layout k_gz_decode reads and writes)
    uint64_t start, stop, slot_off;
    uint32_t cap, first;
    uint32_t status, out_n;
    uint64_t end_bit;
  };
  struct Place {  // (k_gz_chain, k_gz_resolve)
    uint64_t slot_off, out_off;
    uint32_t out_n, valid;
  };
  virtual bool load(const uint8_t* comp, size_t n, bool first) = 0;
  virtual bool find(uint32_t chunk, uint32_t nchunks, uint64_t* starts) = 0;  // starts[1 .. nchunks)
  virtual bool decode(Job* jobs, uint32_t njobs) = 0;
  // chain, resolve, CRC: the bytes to out() + front, their CRC, whether a marker pointed in front of the member
  virtual bool finish(const Place* places, uint32_t m, uint64_t out_n, uint32_t front, uint32_t* crc, bool* bad) = 0;
};

// the bytes a device backend of this shape asks of the allocator
uint64_t gzip_device_bytes(const GzipParams& P);
// nullptr with *why when the buffers cannot be made; `stream`: a hipStream_t (every copy and launch goes on it)
std::unique_ptr<GzipBackend> make_gzip_device_backend(int device, void* stream, const GzipParams& P, std::string* why);
std::unique_ptr<GzipBackend> make_gzip_host_backend(const GzipParams& P);

// the bytes of the gzip member header at p[0, left) (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC, the header CRC checked);
// 0 when it is none, is cut, or is one zlib would refuse
size_t gzip_header_bytes(const uint8_t* p, size_t left);

// A whole gzip file through the backend.  deliver(bytes, n, last): a window's resolved bytes (at backend.out() + front),
// in order, `last` with the file's last ones (which may be none); front() says, before each window, whether a byte is
// held back in front of it.  deliver returns false when it cannot go on (kGzHip).  Returns the outcome; on anything but
// kGzDone the caller forgets what was delivered and reads the file again with zlib.
int gzip_route(const uint8_t* file, size_t n, const GzipParams& P, GzipBackend& backend, GzipStats* stats,
               const std::function<uint32_t()>& front, const std::function<bool(const uint8_t*, uint64_t, bool)>& deliver);

// g2s_reads_set_device_gzip: -1 follows G2S_DEVICE_GZIP (read per call; unset: off), 0 forbids, 1 asks
int set_device_gzip(int mode);
bool device_gzip_asked();
// the switches' values (G2S_GZIP_CHUNK_BYTES, G2S_GZIP_WINDOW_CHUNKS, G2S_GZIP_SLOT_RATIO) over the defaults
GzipParams gzip_params_from_env();

}  // namespace g2s
