// dev.h — HIP device-memory RAII + error plumbing for the engine.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <future>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <stdexcept>
#include <string>
#include <utility>

namespace auron {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    throw HipError(std::string(what) + ": " + hipGetErrorString(e));
  }
}

#define AURON_HIP(call) ::auron::hip_check((call), #call)

// Process-wide caching pools: hipMalloc/hipFree and hipHostMalloc cost
// milliseconds per call on this stack, and a task-per-batch-set workload
// re-allocates identical sizes every task (measured ~180 ms/step of pure
// allocation on the 1B bench before this cache).
class DevPool {
 public:
  static DevPool& inst() {
    static DevPool p;
    return p;
  }

  void* get(size_t size) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = free_.find(size);
    if (it != free_.end() && !it->second.empty()) {
      void* p = it->second.back();
      it->second.pop_back();
      cached_ -= size;
      return p;
    }
    return nullptr;
  }

  // returns true if cached (caller must not free)
  bool put(void* p, size_t size) {
    std::lock_guard<std::mutex> lk(mu_);
    if (cached_ + size > cap_) return false;
    free_[size].push_back(p);
    cached_ += size;
    return true;
  }

  void clear(void (*deleter)(void*)) {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto& [sz, v] : free_)
      for (void* p : v) deleter(p);
    free_.clear();
    cached_ = 0;
  }

 private:
  std::mutex mu_;
  std::unordered_map<size_t, std::vector<void*>> free_;
  size_t cached_ = 0;
  size_t cap_ = 48ull << 30;  // of 288 GB HBM
};

class PinnedPool {
 public:
  static PinnedPool& inst() {
    static PinnedPool p;
    return p;
  }
  void* get(size_t size) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = free_.find(size);
    if (it != free_.end() && !it->second.empty()) {
      void* p = it->second.back();
      it->second.pop_back();
      cached_ -= size;
      return p;
    }
    return nullptr;
  }
  bool put(void* p, size_t size) {
    std::lock_guard<std::mutex> lk(mu_);
    if (cached_ + size > cap_) return false;
    free_[size].push_back(p);
    cached_ += size;
    return true;
  }

 private:
  std::mutex mu_;
  std::unordered_map<size_t, std::vector<void*>> free_;
  size_t cached_ = 0;
  size_t cap_ = 4ull << 30;
};

// Owned device buffer, backed by the caching pool.
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(size_t size) { alloc(size); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr_(o.ptr_), size_(o.size_) {
    o.ptr_ = nullptr;
    o.size_ = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      free();
      ptr_ = o.ptr_;
      size_ = o.size_;
      o.ptr_ = nullptr;
      o.size_ = 0;
    }
    return *this;
  }
  ~DevBuf() { free(); }

  void alloc(size_t size) {
    free();
    if (size == 0) return;
    ptr_ = DevPool::inst().get(size);
    if (!ptr_) AURON_HIP(hipMalloc(&ptr_, size));
    size_ = size;
  }
  void free() {
    if (ptr_) {
      if (!DevPool::inst().put(ptr_, size_)) (void)hipFree(ptr_);
      ptr_ = nullptr;
      size_ = 0;
    }
  }
  void* release() { return std::exchange(ptr_, nullptr); }

  template <typename T = void>
  T* get() const {
    return static_cast<T*>(ptr_);
  }
  size_t size() const { return size_; }
  explicit operator bool() const { return ptr_ != nullptr; }

 private:
  void* ptr_ = nullptr;
  size_t size_ = 0;
};

// Pinned (page-locked) host buffer for small metadata readbacks — pageable
// D2H copies cost milliseconds per call on this stack.
class PinnedBuf {
 public:
  PinnedBuf() = default;
  explicit PinnedBuf(size_t size) { alloc(size); }
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { free(); }

  void alloc(size_t size) {
    free();
    if (size == 0) return;
    ptr_ = PinnedPool::inst().get(size);
    if (!ptr_) AURON_HIP(hipHostMalloc(&ptr_, size));
    size_ = size;
  }
  void free() {
    if (ptr_) {
      if (!PinnedPool::inst().put(ptr_, size_)) (void)hipHostFree(ptr_);
      ptr_ = nullptr;
      size_ = 0;
    }
  }
  // forget the allocation without freeing (static-destruction teardown:
  // hipHostFree after HIP runtime exit crashes)
  void* release() {
    size_ = 0;
    return std::exchange(ptr_, nullptr);
  }
  template <typename T = void>
  T* get() const {
    return static_cast<T*>(ptr_);
  }
  size_t size() const { return size_; }

 private:
  void* ptr_ = nullptr;
  size_t size_ = 0;
};

// Owning, move-only host byte buffer for exported columns (values, validity
// bitmaps, offsets). Pinned and pool-backed, so a D2H copy lands straight in
// the memory that is handed to the consumer; the Arrow release callback gives
// it back to the pool. Capacities are rounded up so that output batches of
// varying length share pool entries: to a power of two up to 1 MiB (4 KiB at
// least), to a whole MiB above, which keeps the pinned excess of a large
// column below 1 MiB.
class HostBuf {
 public:
  HostBuf() = default;
  explicit HostBuf(size_t size) { alloc(size); }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : ptr_(o.ptr_), size_(o.size_), cap_(o.cap_) {
    o.ptr_ = nullptr;
    o.size_ = o.cap_ = 0;
  }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) {
      free();
      ptr_ = o.ptr_;
      size_ = o.size_;
      cap_ = o.cap_;
      o.ptr_ = nullptr;
      o.size_ = o.cap_ = 0;
    }
    return *this;
  }
  ~HostBuf() { free(); }

  // size 0 still allocates: an exported Arrow buffer pointer must not be null
  void alloc(size_t size) {
    free();
    constexpr size_t MIB = (size_t)1 << 20;
    size_t cap = 4096;
    while (cap < size && cap < MIB) cap <<= 1;
    if (cap < size) cap = (size + MIB - 1) / MIB * MIB;
    ptr_ = PinnedPool::inst().get(cap);
    if (!ptr_) AURON_HIP(hipHostMalloc(&ptr_, cap));
    size_ = size;
    cap_ = cap;
  }
  void free() {
    if (ptr_) give_back(ptr_, cap_);
    ptr_ = nullptr;
    size_ = cap_ = 0;
  }
  // hand the allocation to another owner, who returns it with give_back()
  void* release(size_t* cap) {
    *cap = cap_;
    size_ = cap_ = 0;
    return std::exchange(ptr_, nullptr);
  }
  static void give_back(void* p, size_t cap) {
    if (!PinnedPool::inst().put(p, cap)) (void)hipHostFree(p);
  }
  // the one place a host copy of column payload is made (two output columns
  // over one source); *copied is the caller's byte counter
  HostBuf clone(int64_t* copied) const {
    HostBuf c;
    if (!ptr_) return c;
    c.alloc(size_);
    memcpy(c.ptr_, ptr_, size_);
    *copied += (int64_t)size_;
    return c;
  }

  template <typename T = uint8_t>
  T* as() const {
    return static_cast<T*>(ptr_);
  }
  uint8_t* data() const { return static_cast<uint8_t*>(ptr_); }
  size_t size() const { return size_; }
  bool empty() const { return ptr_ == nullptr; }

 private:
  void* ptr_ = nullptr;
  size_t size_ = 0, cap_ = 0;
};

// Double-buffered pinned upload: hipMemcpyAsync from PAGEABLE memory blocks
// while the runtime stages it (~3-5 GB/s end to end); staging through pinned
// chunks overlaps the host memcpy of chunk N+1 with the DMA of chunk N.
// Process-wide like the pools; the mutex serializes callers and the events
// guard pinned-buffer reuse across streams.
class PinnedUploader {
 public:
  static PinnedUploader& inst() {
    static PinnedUploader u;
    return u;
  }

  // the singleton outlives every engine object and is destroyed during
  // static teardown, possibly after the HIP runtime has shut down —
  // hipHostFree/hipEventDestroy there segfault (observed as a core dump at
  // smoke()'s exit). Leak the two 16 MB staging buffers instead; the
  // process is exiting.
  ~PinnedUploader() {
    for (auto& b : bufs_) (void)b.pin.release();
  }

  void copy(void* dst, const void* src, size_t len, hipStream_t s) {
    if (len == 0) return;
    if (len < (256u << 10)) {  // small copies: staging overhead dominates
      AURON_HIP(hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, s));
      return;
    }
    std::lock_guard<std::mutex> lk(mu_);
    constexpr size_t CH = 64u << 20;
    size_t off = 0;
    while (off < len) {
      size_t take = len - off < CH ? len - off : CH;
      Buf& b = bufs_[cur_];
      if (!b.pin.get()) {
        b.pin.alloc(CH);
        AURON_HIP(hipEventCreate(&b.ev));
      } else {
        AURON_HIP(hipEventSynchronize(b.ev));
      }
      // the staging memcpy is the CPU cost of every big upload (a 10 GB
      // parquet scan moves the whole compressed file through here); slice
      // it across a few threads — single-threaded it ran at ~10 GB/s and
      // serialized the scan's host side
      parallel_memcpy(b.pin.get(), (const uint8_t*)src + off, take);
      AURON_HIP(hipMemcpyAsync((uint8_t*)dst + off, b.pin.get(), take,
                               hipMemcpyHostToDevice, s));
      AURON_HIP(hipEventRecord(b.ev, s));
      off += take;
      cur_ ^= 1;
    }
  }

  static void parallel_memcpy(void* dst, const void* src, size_t n) {
    if (n < (8u << 20)) {
      memcpy(dst, src, n);
      return;
    }
    constexpr int T = 8;
    size_t slice = (n + T - 1) / T;
    std::future<void> fs[T];
    for (int t = 0; t < T; t++) {
      size_t lo = (size_t)t * slice;
      size_t hi = lo + slice < n ? lo + slice : n;
      if (lo >= hi) break;
      fs[t] = std::async(std::launch::async, [=] {
        memcpy((uint8_t*)dst + lo, (const uint8_t*)src + lo, hi - lo);
      });
    }
    for (int t = 0; t < T; t++)
      if (fs[t].valid()) fs[t].get();
  }

 private:
  struct Buf {
    PinnedBuf pin;
    hipEvent_t ev = nullptr;
  };
  Buf bufs_[2];
  int cur_ = 0;
  std::mutex mu_;
};

}  // namespace auron
