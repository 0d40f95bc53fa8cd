// chain_dev.hpp — what the forward panel chain (k_panel.hip) and the backward substitution (k_bwd.hip) both need on the device.
#pragma once
#include "dev_math.hpp"

namespace covgpu {

constexpr int PB = 16;                 // block edge

// Workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every outstanding GLOBAL store to be
// acknowledged (s_waitcnt vmcnt(0): ~1 us per step here, where L / Dinv / y stream out while the factorisation goes on
// and nobody reads them back inside the kernel).
COV_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace covgpu
