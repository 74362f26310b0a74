// call_arena.hpp -- the staging arena of the batched calls: one device buffer and one page-locked mirror in the context, shared by
// every call that stages its inputs, runs its kernels and reads its results back with one copy and one synchronisation.
//   device [in | work | out], mirror [in | out], every part at a multiple of 256 bytes; grown by half on demand, never shrunk.
// Every call ends with the context's stream idle, so the next call finds the arena free: one call at a time per context.
// Users: the loop chain, the ring-key search of many indexes, ICP, distance map, immature points, trace, pixel selection, residual
// linearisation, Hessian accumulation, the window solve, the window step, the window's marginalisation, the window's nullspaces, the window's rescale, the window's admission and dsm_set_refs_from_points with all three regions; dsm_tracker_set_ref, _get_template, _upload_frame and _get_frame with `work` alone
// (their copies go from and to the caller's memory, so `in` and `out` stay empty and only the device buffer grows).
#pragma once
#include "dsm_internal.hpp"

namespace dsm {

class CallArena {
public:
  struct Region { // linear sub-allocation: take() returns the offset of `bytes` more, the next one starts at a multiple of 256
    size_t used = 0;
    size_t take(size_t bytes) {
      const size_t o = used;
      used = (used + bytes + 255) & ~(size_t)255;
      return o;
    }
  };
  Region in, work, out; // staged through the mirror, device only, read back through the mirror: all taken before bind()

  // selects the context's device and grows its buffers to hold the three regions; the accessors below hold from here on
  int bind(dsm_context *ctx);
  template <typename T> T *dev_in(size_t off = 0) const { return (T *)(d_ + off); }
  template <typename T> T *dev_work(size_t off = 0) const { return (T *)(d_ + in.used + off); }
  template <typename T> T *dev_out(size_t off = 0) const { return (T *)(d_ + in.used + work.used + off); }
  template <typename T> T *host_in(size_t off = 0) const { return (T *)(h_ + off); }
  template <typename T> const T *host_out(size_t off = 0) const { return (const T *)(h_ + in.used + off); }
  // the first `bytes` of `in` to the device, on the context's stream
  int upload(size_t bytes) const;
  int upload() const { return upload(in.used); }
  // the first `bytes` of `out` to the mirror (0: no copy), then the stream drained
  int fetch(size_t bytes) const;

private:
  dsm_context *ctx_ = nullptr;
  unsigned char *d_ = nullptr, *h_ = nullptr;
};

// Packs host arrays as 4-byte words into one staged block that the kernels index by word offset (the off_* of TrJob, ImJob, DmJob).
struct WordPacker {
  float *base;
  size_t at = 0;
  void *reserve(int *off, size_t n_words) { // n_words at the current word; its offset into *off (unless null)
    if (off) *off = (int)at;
    at += n_words;
    return base + at - n_words;
  }
  void put(int *off, const void *a, size_t n_words) {
    void *to = reserve(off, n_words);
    if (n_words) memcpy(to, a, 4 * n_words);
  }
  void put2(int *off, const void *a, size_t na, const void *b, size_t nb) { put(off, a, na), put(nullptr, b, nb); } // back to back
};

} // namespace dsm
