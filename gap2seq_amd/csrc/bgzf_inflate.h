// gap2seq_amd/csrc/bgzf_inflate.h — what bam.cpp sees of the device inflate (bgzf_inflate.hip): two slots of buffers,
// each holding one window of BGZF members on its way through the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace g2s {

// one member of a window, as the kernel reads it
struct BgzfMember {
  uint64_t in_off;   // of its deflate bytes in the window's staged input
  uint64_t out_off;  // of its inflated bytes in the window
  uint32_t in_len;   // deflate bytes
  uint32_t isize;    // inflated bytes (its trailer's ISIZE, at most 65 536)
  uint32_t crc;      // its trailer's CRC-32
  uint32_t pad;
};

class BgzfDevice {
 public:
  // Buffers for windows of at most max_in staged bytes, max_out inflated bytes and max_members members; `front` bytes
  // of room in front of every inflated window (for the bytes a reader carries over from the window before).  Null
  // when the device is no usable gfx950 or something could not be allocated: *why says which.
  // host_window false: no page-locked window (a caller whose windows all stay on the device: launch with `down` false)
  static BgzfDevice* create(int device, size_t max_in, size_t max_out, size_t max_members, size_t front, std::string* why,
                            bool host_window = true);
  ~BgzfDevice();
  BgzfDevice(const BgzfDevice&) = delete;
  BgzfDevice& operator=(const BgzfDevice&) = delete;
  // page-locked: the staged input and the member list to fill in, the inflated window and the members' status words
  // (inflate_core.h: kOk ...) to read after wait()
  uint8_t* in(int slot) const { return s_[slot].h_in; }
  BgzfMember* members(int slot) const { return s_[slot].h_mem; }
  uint8_t* window(int slot) const { return s_[slot].h_out + front_; }
  const uint32_t* status(int slot) const { return s_[slot].h_st; }
  size_t front() const { return front_; }
  // the same window in device memory, with the same room in front of it (bam_rows.hip reads it there), and the stream
  // (a hipStream_t) everything of this object runs on
  uint8_t* device_window(int slot) const { return s_[slot].d_out + front_; }
  void* stream() const { return stream_; }
  bool fits(size_t n_members, size_t in_bytes, size_t out_bytes) const {
    return n_members <= cap_members_ && in_bytes <= cap_in_ && out_bytes <= cap_out_;
  }
  // copies up, the kernel, copies down (the status words alone when `down` is false: the window stays on the device):
  // all asynchronous, on the object's own stream.  `d_dst` (with `down` false): the kernel writes the window there, any
  // device address with out_bytes bytes of room, in place of the slot's own buffer.
  bool launch(int slot, size_t n_members, size_t in_bytes, size_t out_bytes, std::string* why, bool down = true,
              uint8_t* d_dst = nullptr);
  bool wait(int slot, std::string* why);
  // the device memory create() takes for the two slots: staged input, the window with its front, member list and
  // status words (create() checks its allocations against this)
  static uint64_t device_bytes(size_t max_in, size_t max_out, size_t max_members, size_t front, bool host_window = true) {
    return 2 * ((uint64_t)max_in + 16 + (host_window ? front + max_out + 64 : 0) + (max_members + 1) * (sizeof(BgzfMember) + 4));
  }

 private:
  BgzfDevice() {}
  struct Slot {
    uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
    BgzfMember *h_mem = nullptr, *d_mem = nullptr;
    uint32_t *h_st = nullptr, *d_st = nullptr;
    void* done = nullptr;  // hipEvent_t
    bool busy = false;
  } s_[2];
  void* stream_ = nullptr;  // hipStream_t
  int device_ = -1;
  size_t front_ = 0, cap_in_ = 0, cap_out_ = 0, cap_members_ = 0;
};

}  // namespace g2s
