// pcg32_device.h — tcnn's pcg32 (EXTERNAL) on the device: the stream the training samplers draw from (neural_sampler.cu:36-41).
// Shared by volume.hip (take_samples_kernel) and guided_sampler.hip (take_samples_weighted_kernel).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace vnr {

struct Pcg32Dev {
  uint64_t state, inc;
  __device__ Pcg32Dev(uint64_t initstate, uint64_t initseq)
  {
    state = 0u; inc = (initseq << 1u) | 1u; next_uint(); state += initstate; next_uint();
  }
  __device__ uint32_t next_uint()
  {
    const uint64_t old = state;
    state = old * 0x5851f42d4c957f2dULL + inc;
    const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((~rot + 1u) & 31));
  }
  __device__ float next_float() { const uint32_t u = (next_uint() >> 9) | 0x3f800000u; return __uint_as_float(u) - 1.0f; }
  __device__ void advance(uint64_t delta)
  {
    uint64_t cm = 0x5851f42d4c957f2dULL, cp = inc, am = 1u, ap = 0u;
    while (delta > 0) {
      if (delta & 1) { am *= cm; ap = ap * cm + cp; }
      cp = (cm + 1) * cp; cm *= cm; delta >>= 1;
    }
    state = am * state + ap;
  }
};

}  // namespace vnr
