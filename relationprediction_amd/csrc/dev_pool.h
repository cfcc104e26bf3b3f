// DevPool: the owner of a set of device allocations.  Host-only; depends on the HIP runtime API, include/rgcn.h and the
// standard library (tests/sanitize/dev_pool_driver.cpp runs it against a fake runtime).
//
// Whoever allocates says which pool owns the block; freeing is pool.release(), one line per owner.  No arena and no
// sub-allocation: every alloc() is one hipMalloc, so addresses, alignment and footprint are what a bare hipMalloc gives.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rgcn.h"

namespace rgcn {

class DevPool {
 public:
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  DevPool(DevPool&& o) noexcept : blocks_(std::move(o.blocks_)), bytes_(o.bytes_) { o.forget(); }
  DevPool& operator=(DevPool&& o) noexcept {
    if (this != &o) {
      release();
      blocks_ = std::move(o.blocks_);
      bytes_ = o.bytes_;
      o.forget();
    }
    return *this;
  }
  ~DevPool() { release(); }

  // One hipMalloc of max(bytes, 1) bytes, recorded; zero: also queue a memset of the block to zero on `stream`.
  // hipErrorOutOfMemory -> RGCN_ERR_NOMEM, any other failure -> RGCN_ERR_HIP, with the reason in *err (may be null).
  // On failure *p is null and nothing is recorded.
  rgcn_status alloc(void** p, size_t bytes, bool zero, hipStream_t stream, std::string* err) {
    return grab(p, bytes ? bytes : 1, bytes, zero, stream, err);
  }
  // the same for n elements of T (n = 0 allocates one element)
  template <class T>
  rgcn_status alloc(T** p, size_t n, bool zero, hipStream_t stream, std::string* err) {
    void* block = nullptr;
    const rgcn_status s = grab(&block, (n ? n : 1) * sizeof(T), n * sizeof(T), zero, stream, err);
    *p = static_cast<T*>(block);
    return s;
  }

  // hipFree of every recorded block, last allocated first; the pool is empty afterwards (a second call frees nothing)
  void release() {
    for (size_t i = blocks_.size(); i-- > 0;) (void)hipFree(blocks_[i].p);
    forget();
  }

  int64_t blocks() const { return (int64_t)blocks_.size(); }   // live blocks
  int64_t bytes() const { return (int64_t)bytes_; }            // ... and their sizes as allocated

 private:
  struct Block {
    void* p;
    size_t size;
  };
  // size: what is allocated; bytes: what the caller asked for (the figure an error message names)
  rgcn_status grab(void** p, size_t size, size_t bytes, bool zero, hipStream_t stream, std::string* err) {
    *p = nullptr;
    void* block = nullptr;
    hipError_t e = hipMalloc(&block, size);
    if (e != hipSuccess) {
      if (err) *err = "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? RGCN_ERR_NOMEM : RGCN_ERR_HIP;
    }
    if (zero && (e = hipMemsetAsync(block, 0, size, stream)) != hipSuccess) {
      if (err) *err = "hipMemsetAsync of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e);
      (void)hipFree(block);
      return RGCN_ERR_HIP;
    }
    blocks_.push_back(Block{block, size});
    bytes_ += size;
    *p = block;
    return RGCN_OK;
  }
  void forget() {
    blocks_.clear();
    bytes_ = 0;
  }
  std::vector<Block> blocks_;
  size_t bytes_ = 0;
};

}  // namespace rgcn
