// cost_key.h -- a cost as the unsigned key of the same order that the selection and the ranking of multistart_kernels.hip compare
// with integer atomics, and the cost of a key: one definition for the device and for the host (multistart.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>

// doubles as unsigned keys of the same order (-0 made +0 first: equal costs must tie)
__host__ __device__ __forceinline__ unsigned long long cost_key(double c)
{
   c += 0.0;
   unsigned long long b;
   memcpy(&b, &c, sizeof(b));
   return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double cost_of_key(unsigned long long key)
{
   const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
   double c;
   memcpy(&c, &b, sizeof(c));
   return c;
}
