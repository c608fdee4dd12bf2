// devbuf.h -- the host layer's handles on a device: the guard that makes a device current, the check of a HIP call, device memory
// with one owner.  Included by batch.h and by the headers that hold device memory without needing the module (hmc.h).
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include <vector>

namespace orc {

// makes `device` the calling thread's current HIP device for the lifetime of the object
// (every entry point of a batch asserts its device: several modules, or the shards of one batch,
// may live on different GPUs of the node inside one process)
class DeviceGuard
{
public:
   explicit DeviceGuard(int device);
   ~DeviceGuard();
   DeviceGuard(const DeviceGuard &) = delete;
   DeviceGuard & operator=(const DeviceGuard &) = delete;
private:
   int prev_ = -1;
   bool changed_ = false;
};

void hip_check(hipError_t e, const char * what);
// device memory released on the device it was allocated on
std::shared_ptr<void> device_buffer(int device, size_t bytes);

// Device memory with one owner: what the handle holds is freed when it is reset or destroyed, on the device that was current
// when the handle took it (the device of the allocation).
class DevBuf
{
public:
   DevBuf() = default;
   ~DevBuf() { reset(); }
   DevBuf(const DevBuf &) = delete;
   DevBuf & operator=(const DevBuf &) = delete;
   void reset(void * p = nullptr);
   template <typename T> T * as() const { return static_cast<T *>(p_); }
   explicit operator bool() const { return p_ != nullptr; }
private:
   void * p_ = nullptr;
   int device_ = -1;
};
// what a DevBuf is reset with: an array of `count` elements (at least one); below, a host vector uploaded as `real`s (waits for the copy)
template <typename T> T * dev_alloc(size_t count)
{
   T * p = nullptr;
   hip_check(hipMalloc((void **) &p, (count ? count : 1) * sizeof(T)), "hipMalloc");
   return p;
}

template <typename real> real * upload(const std::vector<double> & v, hipStream_t s)
{
   std::vector<real> tmp(v.begin(), v.end());
   real * d = dev_alloc<real>(tmp.size());
   hip_check(hipMemcpyAsync(d, tmp.data(), tmp.size() * sizeof(real), hipMemcpyHostToDevice, s), "upload");
   hip_check(hipStreamSynchronize(s), "upload sync");
   return d;
}

} // namespace orc
