// devbuf.cpp -- the definitions of devbuf.h: the check of a HIP call, the device guard, device memory with one owner.
#include "devbuf.h"
#include <stdexcept>
#include <string>

namespace orc {

void hip_check(hipError_t e, const char * what)
{
   if (e != hipSuccess)
      throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

DeviceGuard::DeviceGuard(int device)
{
   if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
   if (prev_ != device)
   {
      hip_check(hipSetDevice(device), "hipSetDevice");
      changed_ = true;
   }
}

DeviceGuard::~DeviceGuard()
{
   if (changed_ && prev_ >= 0) (void) hipSetDevice(prev_);
}

std::shared_ptr<void> device_buffer(int device, size_t bytes)
{
   DeviceGuard guard(device);
   void * p = nullptr;
   hip_check(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc");
   return std::shared_ptr<void>(p, [device](void * q) {
      int prev = -1;
      const bool have = hipGetDevice(&prev) == hipSuccess;
      (void) hipSetDevice(device);
      (void) hipFree(q);
      if (have && prev != device) (void) hipSetDevice(prev);
   });
}

void DevBuf::reset(void * p)
{
   if (p_) { DeviceGuard guard(device_); (void) hipFree(p_); }
   p_ = p; device_ = -1;
   if (p) hip_check(hipGetDevice(&device_), "hipGetDevice");
}

} // namespace orc
